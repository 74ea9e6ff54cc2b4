"""Time the LM-head cross-entropy kernels (csrc/wkv6_ce.hip) and the chunked head built on them, in one process.

Row kernels, bf16 logits [n_rows, 65536] for n_rows in {256, 4096, 49152 where it fits}, forward + backward of the training loss
(mean cross-entropy, then L2Wrap):
  torch    callers.lm_loss(kernels=False): F.cross_entropy + the reference's L2Wrap, torch's own kernels -- the baseline, never this code
  kernels  callers.lm_loss(kernels=True): wkv6_ce_rows_forward_bf16, then wkv6_ce_rows_backward_bf16 through autograd
  fused    mix_op.ce_rows_grad_: one launch, in place (what callers.head_loss runs per chunk; the buffer is not refilled between calls, so
           from the second call on it reads the last gradient as logits: the same bytes move)
Reported: median [min, max] ms over the rounds, and for the two kernel forms the achieved bytes per second against the 3 x n_rows x V x 2
bytes they must move (read, read again, write); `spread` is (max - min) / median of a contender's own rounds; `peak` is
torch.cuda.max_memory_allocated above what was allocated before the call, the logits gradient that torch and kernels return included.

head_loss at C = 2048, V = 65536, rows = 16384, trainable head, chunk_rows in {1024, 4096, 16384}, against the unchunked eager head
(F.linear, then lm_loss(kernels=False)): time of forward + backward and torch.cuda.max_memory_allocated above what was allocated before
the call.  The memory claim -- no [rows, V] tensor besides one chunk -- is asserted from those figures.

Method: tools/timing.py (a few warm-up calls of every contender, --repeats rounds, --iters calls per timing).

    python tools/time_ce_rows.py [--out profiles/ce_rows_time.txt]
"""
import argparse
import os
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
V = 65536


def alternate(contenders, iters, repeats, warm=3):
    """{name: [ms per call, one per round]}; contenders: {name: callable}"""
    import torch
    for fn in contenders.values():
        timing.warm(fn, calls=warm, sync=None)
    torch.cuda.synchronize()
    return timing.alternate(contenders, lambda fn: timing.event_time(fn, iters), repeats)


def fmt(ms):
    med = timing.median(ms)
    return f"{med:9.3f} ms [{min(ms):8.3f}, {max(ms):8.3f}]  spread {100 * (max(ms) - min(ms)) / med:5.1f} %"


def peak_above(fn):
    """bytes of torch.cuda.max_memory_allocated that one call of fn adds to what is allocated before it"""
    import torch
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def row_kernels(n_rows, iters, repeats, say):
    import torch
    from rwkv_lm_ext_amd import callers, mix_op
    gen = torch.Generator(device="cuda").manual_seed(n_rows)
    z = (torch.randn(n_rows, V, device="cuda", generator=gen) * 4).bfloat16().requires_grad_()
    t = torch.randint(0, V, (n_rows,), device="cuda", generator=gen)
    buf = z.detach().clone()
    ce, l2 = torch.full((n_rows,), 1.0 / n_rows, device="cuda"), torch.full((n_rows,), 1e-4 / n_rows, device="cuda")

    def run(kernels):
        def fn():
            z.grad = None
            callers.lm_loss(z.view(1, n_rows, V), t.view(1, n_rows), kernels=kernels).backward()
        return fn

    contenders = {"torch": run(False), "kernels": run(True), "fused": lambda: mix_op.ce_rows_grad_(buf, t, ce, l2)}
    peaks = {}
    for name, fn in contenders.items():
        z.grad = None                                      # every contender starts without the gradient the one before it left
        peaks[name] = peak_above(fn)
    times = alternate(contenders, iters, repeats)
    must = 3 * n_rows * V * 2
    say(f"n_rows = {n_rows}, V = {V}, bf16 (logits {n_rows * V * 2 / 2 ** 30:.2f} GiB)")
    for name, ms in times.items():
        rate = "" if name == "torch" else f"  {must / timing.median(ms) * 1e-9:7.3f} TB/s of the {must / 2 ** 30:.2f} GiB that must move"
        say(f"  {name:8s} {fmt(ms)}  peak +{peaks[name] / 2 ** 30:6.2f} GiB{rate}")
    med = {name: timing.median(ms) for name, ms in times.items()}
    margin = max(times["torch"]) - min(times["torch"]) + max(times["kernels"]) - min(times["kernels"])
    say(f"  torch / kernels = {med['torch'] / med['kernels']:.2f}x, torch / fused = {med['torch'] / med['fused']:.2f}x; "
        f"kernels below torch by more than both spreads: {med['torch'] - med['kernels'] > margin}")
    return med["torch"] - med["kernels"] > margin


def head(rows, C, iters, repeats, say):
    import torch
    import torch.nn.functional as F
    from rwkv_lm_ext_amd import callers
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = (torch.randn(rows, C, device="cuda", generator=gen)).bfloat16().requires_grad_()
    W = (torch.randn(V, C, device="cuda", generator=gen) * 0.02).bfloat16().requires_grad_()
    t = torch.randint(0, V, (rows,), device="cuda", generator=gen)

    def clear():
        x.grad = W.grad = None

    def eager():
        clear()
        callers.lm_loss(F.linear(x, W).view(1, rows, V), t.view(1, rows), kernels=False).backward()

    def chunked(chunk_rows):
        def fn():
            clear()
            callers.head_loss(x, W, t, chunk_rows=chunk_rows, kernels=True).backward()
        return fn

    contenders = {"eager head": eager}
    contenders.update({f"head_loss {c}": chunked(c) for c in (1024, 4096, 16384)})
    peaks = {}
    for name, fn in contenders.items():
        peaks[name] = peak_above(fn)
        clear()
    times = alternate(contenders, iters, repeats, warm=2)
    clear()
    say(f"head: rows = {rows}, C = {C}, V = {V}, bf16, trainable head (logits would be {rows * V * 2 / 2 ** 30:.2f} GiB)")
    for name, ms in times.items():
        say(f"  {name:16s} {fmt(ms)}  peak +{peaks[name] / 2 ** 30:6.2f} GiB")
    # the claim: one chunk of logits, gx, the fp32 gW and its bf16 copies (the stored one, the scaled one, the .grad), small change
    for c in (1024, 4096, 16384):
        bound = min(c, rows) * V * 2 + 2 * rows * C * 2 + V * C * (4 + 4 + 3 * 2) + (64 << 20)
        ok = peaks[f"head_loss {c}"] <= bound
        say(f"  chunk_rows {c}: peak {peaks[f'head_loss {c}'] / 2 ** 30:.2f} GiB <= one chunk + gx + gW = {bound / 2 ** 30:.2f} GiB: {ok}")
        assert ok, "head_loss held more than one chunk of logits"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rows", type=int, nargs="*", default=[256, 4096, 49152])
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "no GPU: nothing is measured on a CPU"
    torch.set_num_threads(min(16, torch.get_num_threads()))
    log = timing.Log()
    say = log.say

    p = torch.cuda.get_device_properties(0)
    say(f"# tools/time_ce_rows.py on {p.name}, {p.multi_processor_count} CUs, torch {torch.__version__}, HIP {torch.version.hip}; one box, one run")
    say(f"# {args.repeats} alternating rounds of {args.iters} calls each, device events; median [min, max]")
    free = torch.cuda.mem_get_info()[0]
    wins = {}
    for n_rows in args.rows:
        if n_rows * V * 2 * 7 > free:                       # torch's own path keeps about six times the logits
            say(f"n_rows = {n_rows}: does not fit ({free / 2 ** 30:.0f} GiB free), not measured")
            continue
        wins[n_rows] = row_kernels(n_rows, args.iters if n_rows > 1000 else 10 * args.iters, args.repeats, say)
        torch.cuda.empty_cache()
    say(f"lm_loss(kernels=None) may choose the kernels at n_rows {[n for n, w in wins.items() if w]}, not at {[n for n, w in wins.items() if not w]}")
    head(16384, 2048, max(1, args.iters // 2), args.repeats, say)
    log.write(args.out and os.path.join(ROOT, args.out))          # (a relative --out is under the repository; join keeps an absolute one)


if __name__ == "__main__":
    main()
