"""Time the device-side sampler (mix_op.sample_slots: one rwkv6_sample_slots_bf16 launch, csrc/wkv6_sample.hip) on bf16 logits rows of
V = 65536 for n_seq in {1, 8, 256}, under three settings -- top-p 0.85 (top-k off), top-k 50 (top-p off), greedy -- all with presence /
frequency penalties and a decaying occurrence pool of 256 slots, eagerly and replayed from a captured graph.

Baseline ('torch'): what a caller of the parent commit has behind the head -- a batched sampler of torch ops written here (gather of the
pool rows, penalties, softmax over a full descending sort, cumsum, nucleus / top-k mask, inverse CDF in sorted order, scatter-update of the
pool).  It reads nothing on the host, so that it can be captured too.

Method: tools/timing.py, in one child process per n_seq, started fresh and ended by a time limit of its own (--limit seconds), at most 16
threads (--warm seconds of warm-up each, synchronised after every call; --repeats rounds of the two; --iters calls per timing); reported is
the median [min, max] over the rounds.  The last lines state the kernel's
time as a share of the graph-replayed decode step of 256 sequences that tools/time_packed_step.py recorded (profiles/packed_step_time.txt).

    python tools/time_sample_slots.py [--out profiles/sample_slots_time.txt]
"""
import argparse
import os
import re
import subprocess
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, N_SLOTS = 65536, 256
N_SEQ = (1, 8, 256)
SETTINGS = {"top-p 0.85": dict(temperature=1.0, top_p=0.85, top_k=0), "top-k 50": dict(temperature=1.0, top_p=1.0, top_k=50),
            "greedy": dict(temperature=0.0, top_p=1.0, top_k=0)}
PENALTIES = dict(alpha_presence=0.3, alpha_frequency=0.3, alpha_decay=0.996)


def torch_sampler(logits, occ, slots, params, u):
    import torch
    x = logits.float()
    o = occ[slots]
    temp, top_p, top_k, ap, af, decay = (params[:, i:i + 1] for i in range(6))
    z = torch.where(o > 0, x - (ap + o * af), x)
    zs, idx = torch.sort(z, dim=1, descending=True)
    cum = torch.softmax(zs, 1).cumsum(1)
    cut = zs.gather(1, (cum >= top_p).float().argmax(1, keepdim=True))
    keep = (zs >= cut) | (top_p >= 1)
    keep &= (torch.arange(z.shape[1], device=z.device).unsqueeze(0) < top_k) | (top_k == 0)
    greedy = temp == 0
    w = torch.exp((zs - zs[:, :1]) / torch.where(greedy, torch.ones_like(temp), temp)) * keep
    cdf = w.cumsum(1)
    pick = (cdf > u.unsqueeze(1) * cdf[:, -1:]).float().argmax(1, keepdim=True)
    tok = idx.gather(1, torch.where(greedy, torch.zeros_like(pick), pick))
    occ[slots] = (o * decay).scatter_add_(1, tok, torch.ones_like(tok, dtype=torch.float32))
    return tok.squeeze(1).int()


def worker(n_seq, iters, repeats, warm):
    sys.path.insert(0, ROOT)
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from rwkv_lm_ext_amd import infctx, mix_op
    torch.manual_seed(0)
    logits = (torch.randn(n_seq, V, device="cuda") * 2).bfloat16()
    slots = torch.randperm(N_SLOTS, device="cuda")[:n_seq].int()
    u = torch.rand(n_seq, device="cuda")
    timing.emit(timing.device_record())

    def graphed(fn):
        replay, kept = timing.graphed(fn)
        return lambda: (replay(), kept)[1]

    with torch.no_grad():
        for name, setting in SETTINGS.items():
            params = infctx.sampling_params(n_seq, "cuda", **setting, **PENALTIES)
            pools = [(torch.rand(N_SLOTS, V, device="cuda") < 0.01).float() * 1.5 for _ in range(2)]
            long_slots = slots.long()
            kernel = lambda: mix_op.sample_slots(logits, pools[0], slots, params, u)
            torch_ = lambda: torch_sampler(logits, pools[1], long_slots, params, u)
            same = (kernel() == torch_()).float().mean().item()      # (the two draw in different orders: equal for greedy only)
            for graph in (False, True):
                fns = {"kernel": graphed(kernel) if graph else kernel, "torch": graphed(torch_) if graph else torch_}
                for fn in fns.values():
                    timing.warm(fn, seconds=warm, sync="each")
                res = timing.alternate(fns, lambda fn: timing.event_time(fn, iters) * 1e3, repeats)
                timing.emit({"setting": name, "graph": graph, "us": res, "same_tokens": same})
    timing.emit({"done": True})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warm", type=float, default=0.3)
    ap.add_argument("--limit", type=float, default=150.0, help="seconds a child process (one n_seq) may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", type=int, default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.iters, a.repeats, a.warm)
    log = timing.Log()
    say = log.say
    env = dict(os.environ, OMP_NUM_THREADS=str(min(16, int(os.environ.get("OMP_NUM_THREADS", "16")))))
    graph_kernel_256 = {}
    for n_seq in N_SEQ:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", str(n_seq), "--iters", str(a.iters), "--repeats", str(a.repeats),
               "--warm", str(a.warm)]
        try:
            out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, cwd=ROOT, env=env, timeout=a.limit)
        except subprocess.TimeoutExpired:
            say(f"n_seq = {n_seq}: the child process passed its limit of {a.limit:.0f} s and was ended; nothing after it is run")
            break
        rows = timing.records(out.stdout)
        if out.returncode != 0 or not rows or not rows[-1].get("done"):
            say(f"n_seq = {n_seq}: the child process failed (exit code {out.returncode}); nothing after it is run")
            break
        if not log.lines:
            say(timing.device_header(rows[0]))
            say(f"bf16 logits [n_seq, {V}], occurrence pool fp32 [{N_SLOTS}, {V}] with 1 % of its entries set, penalties {PENALTIES}; "
                f"{a.iters} calls per timing, {a.repeats} alternated rounds, {a.warm:.1f} s warm-up each; us per call: median [min, max]")
            say("kernel: mix_op.sample_slots (one launch).  torch: the batched sort-based sampler of torch ops in tools/time_sample_slots.py.")
            say()
        say(f"n_seq = {n_seq}")
        for r in rows[1:-1]:
            k, t = r["us"]["kernel"], r["us"]["torch"]
            mk, mt = timing.median(k), timing.median(t)
            clear = "ranges do not overlap" if timing.apart(k, t) else "RANGES OVERLAP"
            say(f"  {r['setting']:10s} {'graph' if r['graph'] else 'eager'}  kernel {mk:9.1f} [{min(k):9.1f}, {max(k):9.1f}]   torch {mt:9.1f} "
                f"[{min(t):9.1f}, {max(t):9.1f}]   kernel / torch = {mk / mt:.3f} ({clear}); torch's spread {max(t) - min(t):.1f}")
            if n_seq == 256 and r["graph"]:
                graph_kernel_256[r["setting"]] = mk
        say()
    step = None
    try:
        text = open(os.path.join(ROOT, "profiles", "packed_step_time.txt")).read()
        step = float(re.search(r"\(i\) 256 x 1, n_slots = 256\n(?:.*\n)*?\s*step x24\s+graph\s+new\s+([0-9.]+)", text).group(1))
    except (OSError, AttributeError):
        say("profiles/packed_step_time.txt has no graph-replayed decode step of 256 sequences: the share is not stated")
    if step and graph_kernel_256:
        say(f"share of the graph-replayed 24-layer decode step of 256 sequences ({step:.1f} us, profiles/packed_step_time.txt; head GEMM not "
            "included in either):")
        for name, us in graph_kernel_256.items():
            say(f"  {name:10s} kernel {us:9.1f} us = {100 * us / step:.2f} % of the step")
    log.write(a.out)


if __name__ == "__main__":
    main()
