"""Time the block-level serving step on a packed stateful batch (infctx.block_forward_packed, infctx.step_packed over 24 layers) with the
token-shift state in a device-side slot pool (wkv6_ddlerp_slots_forward + wkv6_shift_keep) against the parent commit, whose
tmix_forward_packed / cmix_forward_packed keep that state with eager torch.  bf16, C = 2048, H = 32, dim_ffn = 7168:

  (i)   a decode step of 256 sequences
  (ii)  8 prompts of 66..512 tokens + 56 decode tokens
  (iii) 8 prompts of 1024 tokens with a snapshot every 256

each at n_slots = 256 and 4096, eagerly and replayed from a captured graph.

Baseline: --parent-tree PATH names a checkout of the parent commit with its own built library; it is imported in a child process started
fresh (this tool never replaces a process image).  The parent has no step_packed: the child loops its tmix_forward_packed /
cmix_forward_packed itself, with the same residual adds and LayerNorms.  Without --parent-tree the baseline is this tree with
pool_kernels=False (the same eager code, kept as the fallback), and the output says so.

Method: tools/timing.py, one child process per side (--warm seconds of warm-up each, synchronised after every call; --repeats rounds;
--iters-block / --iters-step calls per timing); reported is the median [min, max] over the rounds.  The kernel launches per sub-layer come
from a torch.profiler trace taken in child processes of their own, after the timing ones have ended.

    python tools/time_packed_step.py [--parent-tree PATH] [--out profiles/packed_step_time.txt]
"""
import argparse
import functools
import os
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, H, DIM_FFN, LAYERS = 2048, 32, 7168, 24
CASES = {
    "(i) 256 x 1": dict(lens=[1] * 256, snap_every=0),
    "(ii) 8 x 66..512 + 56 x 1": dict(lens=[66 + (i * (512 - 66)) // 7 for i in range(8)] + [1] * 56, snap_every=0),
    "(iii) 8 x 1024, snapshot every 256": dict(lens=[1024] * 8, snap_every=256),
}
N_SLOTS = (256, 4096)


# ---- a child: one side (one tree) in one process, driven over stdin / stdout
def worker(tree, layers):
    sys.path.insert(0, tree)
    import torch
    from rwkv_lm_ext_amd import infctx, train_dp
    assert os.path.abspath(infctx.__file__).startswith(os.path.abspath(tree) + os.sep), infctx.__file__
    bf = torch.bfloat16
    has_step = hasattr(infctx, "step_packed")
    torch.manual_seed(0)
    with torch.device("cuda"):
        blocks = [train_dp.Block(C, C, DIM_FFN, i) for i in range(layers)]
    for b in blocks:
        for p in b.parameters():
            torch.nn.init.normal_(p, 0.0, 0.02)
        b.to(bf).requires_grad_(False)
    i32 = lambda v: torch.tensor(list(v), dtype=torch.int32, device="cuda")
    state = {}

    def setup(case, n_slots):
        state.clear()
        torch.cuda.empty_cache()
        d = CASES[case]
        lens = d["lens"]
        n, total = len(lens), sum(lens)
        cu = [0]
        for m in lens:
            cu.append(cu[-1] + m)
        snap = None
        if d["snap_every"]:
            per = [m // d["snap_every"] for m in lens]
            cs = [0]
            for m in per:
                cs.append(cs[-1] + m)
            assert n + cs[-1] <= n_slots
            snap = (d["snap_every"], i32(cs), i32(range(n, n + cs[-1])))
        state.update(x=torch.randn(1, total, C, device="cuda").to(bf), cu=i32(cu), max_seqlen=max(lens), slots=i32(range(n)), snap=snap,
                     shift_att=torch.zeros(layers, n_slots, C, device="cuda", dtype=bf),
                     shift_ffn=torch.zeros(layers, n_slots, C, device="cuda", dtype=bf),
                     wkv=torch.zeros(layers, n_slots, H, 64, 64, device="cuda"), graphs={})

    def run(n_layers, pool_kernels):
        s = state
        kw = {} if pool_kernels is None else {"pool_kernels": pool_kernels}
        if has_step and pool_kernels is None:
            pools = infctx.PackedPools(s["shift_att"], s["shift_ffn"], s["wkv"])
            if n_layers == 1:
                return infctx.block_forward_packed(blocks[0], s["x"], s["cu"], s["max_seqlen"], pools, 0, s["slots"], snap=s["snap"])
            return infctx.step_packed(blocks[:n_layers], s["x"], s["cu"], s["max_seqlen"], pools, s["slots"], snap=s["snap"])
        x = s["x"]                                      # the parent's functions (or this tree's with pool_kernels=False), looped here
        for i, b in enumerate(blocks[:n_layers]):
            if getattr(b, "ln0", None) is not None:
                x = b.ln0(x)
            x = x + infctx.tmix_forward_packed(b.att, b.ln1(x), s["cu"], s["max_seqlen"], s["shift_att"][i], s["wkv"][i], s["slots"],
                                               snap=s["snap"], **kw)
            x = x + infctx.cmix_forward_packed(b.ffn, b.ln2(x), s["cu"], s["shift_ffn"][i], s["slots"], snap=s["snap"], **kw)
        return x

    def contender(n_layers, pool_kernels, graph):
        if not graph:
            return lambda: run(n_layers, pool_kernels)
        key = (n_layers, pool_kernels)
        if key not in state["graphs"]:
            state["graphs"][key] = timing.graphed(lambda: run(n_layers, pool_kernels))      # (the replay, and the output it writes)
        return state["graphs"][key][0]

    def count(pool_kernels):
        """device operations (kernels, copies, memsets) of one time-mix and one channel-mix sub-layer call, from a profiler trace"""
        from torch.profiler import ProfilerActivity, profile
        from torch.autograd import DeviceType
        s, b, kw = state, blocks[0], {} if pool_kernels is None else {"pool_kernels": pool_kernels}
        calls = {"tmix": lambda: infctx.tmix_forward_packed(b.att, s["x"], s["cu"], s["max_seqlen"], s["shift_att"][0], s["wkv"][0], s["slots"],
                                                           snap=s["snap"], **kw),
                 "cmix": lambda: infctx.cmix_forward_packed(b.ffn, s["x"], s["cu"], s["shift_ffn"][0], s["slots"], snap=s["snap"], **kw)}
        out = {}
        for name, fn in calls.items():
            fn()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            out[name] = sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)
        return out

    ops = {
        "setup": setup,
        "warm": lambda layers, pool_kernels, graph, seconds: timing.warm(contender(layers, pool_kernels, graph), seconds=seconds, sync="each"),
        "time": lambda layers, pool_kernels, graph, iters: {"us": timing.event_time(contender(layers, pool_kernels, graph), iters) * 1e3},
        "count": lambda pool_kernels: {"count": count(pool_kernels)},
    }
    with torch.no_grad():
        timing.serve({"ready": True, "has_step": has_step, **timing.device_record()}, ops)


def child(tree, layers):
    return timing.Child([os.path.abspath(__file__), "--worker", "--tree", tree, "--layers", str(layers)], cwd=tree)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--layers", type=int, default=LAYERS)
    ap.add_argument("--iters-block", type=int, default=20)
    ap.add_argument("--iters-step", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warm", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    if a.worker:
        return worker(os.path.abspath(a.tree), a.layers)
    log = timing.Log()
    say = log.say
    base_tree = os.path.abspath(a.parent_tree) if a.parent_tree else ROOT
    base_kernels = None if a.parent_tree else False    # the parent tree has no such argument; this tree's eager code is pool_kernels=False
    sides = {"new": (ROOT, None), "base": (base_tree, base_kernels)}
    kids = {n: child(tree, a.layers) for n, (tree, _) in sides.items()}
    try:
        say(timing.device_header(kids["new"].hello))
        if a.parent_tree:
            assert not kids["base"].hello["has_step"], "--parent-tree already has step_packed: not the parent commit"
            say("baseline ('base'): the parent commit's tree in a process of its own, its tmix_forward_packed / cmix_forward_packed looped with the "
                "same residual adds and LayerNorms")
        else:
            say("baseline ('base'): NO PARENT TREE GIVEN -- this tree with pool_kernels=False (the parent's eager code, kept as the fallback), looped "
                "the same way, in a process of its own")
        say(f"'new': infctx.block_forward_packed / step_packed of this tree (slot-pool kernels).  bf16, C={C}, H={H}, dim_ffn={DIM_FFN}, "
            f"step = {a.layers} layers; {a.iters_block} (block) / {a.iters_step} (step) calls per timing, {a.repeats} alternated repeats, "
            f"{a.warm:.1f} s warm-up each; times in us per call: median [min, max]")
        say()
        summary = []
        for case in CASES:
            for n_slots in N_SLOTS:
                for k in kids.values():
                    k.ask(op="setup", case=case, n_slots=n_slots)
                say(f"{case}, n_slots = {n_slots}")
                for what, layers, iters in (("block", 1, a.iters_block), (f"step x{a.layers}", a.layers, a.iters_step)):
                    for graph in (False, True):
                        ask = {n: functools.partial(k.ask, layers=layers, pool_kernels=sides[n][1], graph=graph) for n, k in kids.items()}
                        for q in ask.values():
                            q(op="warm", seconds=a.warm)
                        res = timing.alternate(ask, lambda q: q(op="time", iters=iters)["us"], a.repeats)
                        m = {n: timing.median(xs) for n, xs in res.items()}
                        fmt = lambda n: f"{n} {m[n]:10.1f} [{min(res[n]):10.1f}, {max(res[n]):10.1f}]"
                        apart = "ranges do not overlap" if timing.apart(res["new"], res["base"]) else "ranges overlap"
                        mode = "graph" if graph else "eager"
                        say(f"  {what:9s} {mode:5s}  {fmt('new')}   {fmt('base')}   new / base = {m['new'] / m['base']:.3f} ({apart})")
                        summary.append(f"{case}, n_slots {n_slots}, {what}, {mode}: {m['new']:.1f} against {m['base']:.1f} us = "
                                       f"{m['new'] / m['base']:.3f} ({apart})")
                say()
        for s in summary:
            say(s)
    finally:
        for k in kids.values():
            k.close()
    # launches per sub-layer: a run of its own per side (one layer is enough), after the timing processes have ended
    say()
    say("device operations (kernels, copies, memsets) per sub-layer call, from a torch.profiler trace in a process of its own:")
    for n, (tree, pool_kernels) in sides.items():
        k = child(tree, 1)
        try:
            for case in CASES:
                for n_slots in N_SLOTS[:1]:
                    k.ask(op="setup", case=case, n_slots=n_slots)
                    try:
                        c = k.ask(op="count", pool_kernels=pool_kernels)["count"]
                        say(f"  {n:4s} {case}: time-mix {c['tmix']}, channel-mix {c['cmix']}")
                    except RuntimeError as e:
                        say(f"  {n:4s} {case}: not measured ({e})")
        finally:
            k.close()
    log.write(a.out)


if __name__ == "__main__":
    main()
