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

Method of tools/time_rwkv6_split.py: everything is allocated first, each contender is warmed for --warm seconds, then --repeats rounds
alternate the two sides (one child process each, only one of them running at a time), each timing --iters back-to-back calls with device
events; reported is the median [min, max] over the rounds.  The kernel launches per sub-layer come from a torch.profiler trace taken in
child processes of their own, after the timing ones have ended.

    python tools/time_packed_step.py [--parent-tree PATH] [--out profiles/packed_step_time.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, H, DIM_FFN, LAYERS = 2048, 32, 7168, 24
CASES = {
    "(i) 256 x 1": dict(lens=[1] * 256, snap_every=0),
    "(ii) 8 x 66..512 + 56 x 1": dict(lens=[66 + (i * (512 - 66)) // 7 for i in range(8)] + [1] * 56, snap_every=0),
    "(iii) 8 x 1024, snapshot every 256": dict(lens=[1024] * 8, snap_every=256),
}
N_SLOTS = (256, 4096)
TAG = "@@ "


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
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                run(n_layers, pool_kernels)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    state["keep", key] = run(n_layers, pool_kernels)
            torch.cuda.current_stream().wait_stream(side)
            state["graphs"][key] = g
        return state["graphs"][key].replay

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters * 1e3

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

    print(TAG + json.dumps({"ready": True, "has_step": has_step, "device": torch.cuda.get_device_properties(0).name,
                            "cus": torch.cuda.get_device_properties(0).multi_processor_count, "torch": torch.__version__,
                            "hip": torch.version.hip}), flush=True)
    with torch.no_grad():
        for line in sys.stdin:
            q = json.loads(line)
            try:
                if q["op"] == "quit":
                    break
                if q["op"] == "setup":
                    setup(q["case"], q["n_slots"])
                    r = {}
                elif q["op"] == "warm":
                    fn = contender(q["layers"], q["pool_kernels"], q["graph"])
                    t0 = time.time()
                    while time.time() - t0 < q["seconds"]:
                        fn()
                        torch.cuda.synchronize()
                    r = {}
                elif q["op"] == "time":
                    r = {"us": timed(contender(q["layers"], q["pool_kernels"], q["graph"]), q["iters"])}
                elif q["op"] == "count":
                    r = {"count": count(q["pool_kernels"])}
                else:
                    raise ValueError(q["op"])
            except Exception as e:                      # reported, not hidden: the parent of this process prints it and stops
                r = {"error": f"{type(e).__name__}: {e}"}
            print(TAG + json.dumps(r), flush=True)


class Child:
    def __init__(self, tree, layers):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree, "--layers", str(layers)],
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=tree)
        self.hello = self.read()

    def read(self):
        for line in self.p.stdout:
            if line.startswith(TAG):
                r = json.loads(line[len(TAG):])
                if "error" in r:
                    raise RuntimeError(r["error"])
                return r
        raise RuntimeError(f"the child process ended (exit code {self.p.wait()})")

    def ask(self, **q):
        self.p.stdin.write(json.dumps(q) + "\n")
        self.p.stdin.flush()
        return self.read()

    def close(self):
        try:
            self.p.stdin.write(json.dumps({"op": "quit"}) + "\n")
            self.p.stdin.close()
        except OSError:
            pass
        self.p.wait()


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
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    base_tree = os.path.abspath(a.parent_tree) if a.parent_tree else ROOT
    base_kernels = None if a.parent_tree else False    # the parent tree has no such argument; this tree's eager code is pool_kernels=False
    sides = {"new": (ROOT, None), "base": (base_tree, base_kernels)}
    kids = {n: Child(tree, a.layers) for n, (tree, _) in sides.items()}
    try:
        h = kids["new"].hello
        say(f"device: {h['device']}, {h['cus']} CUs; torch {h['torch']}; hip {h['hip']}")
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
                        res = {n: [] for n in kids}
                        for n, k in kids.items():
                            k.ask(op="warm", layers=layers, pool_kernels=sides[n][1], graph=graph, seconds=a.warm)
                        for _ in range(a.repeats):
                            for n, k in kids.items():
                                res[n].append(k.ask(op="time", layers=layers, pool_kernels=sides[n][1], graph=graph, iters=iters)["us"])
                        m = {n: statistics.median(xs) for n, xs in res.items()}
                        fmt = lambda n: f"{n} {m[n]:10.1f} [{min(res[n]):10.1f}, {max(res[n]):10.1f}]"
                        apart = ("ranges do not overlap" if max(res["new"]) < min(res["base"]) or min(res["new"]) > max(res["base"])
                                 else "ranges overlap")
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
        k = Child(tree, 1)
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
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
