"""Time the packed stateful inference call with state snapshots and a separate output slot (rwkv6_forward_varlen_snap_bf16) against what
serves the same request without it, bf16, H=32, C=2048:

  (a) snapshots      8 prompts of 1024 tokens, the state kept every 256 tokens (four snapshots each): one snap call against the chain of four
                     packed calls of 8 x 256 tokens, each starting from the state the one before left (the copies that would move each
                     piece's state out of the slot are left out of the chain: they would only add to it)
  (b) their cost     the same snap call against the single packed call on 8 x 1024, which leaves no snapshot: the difference is what the
                     snapshot stores cost (8 x 4 x 512 KB in the pool's layout)
  (c) output slots   8 sequences of 512 tokens that start from cached slots and leave their state elsewhere: one snap call against
                     pool[dst] = pool[src] followed by the packed call in place on dst

The baselines go to --parent-lib (a librwkv6_amd.so built from the commit before the snap call existed), else to this tree's library.
Method: tools/timing.py (ctypes calls with pre-bound arguments on both sides, a bits check first, --warm seconds of warm-up each, --repeats
rounds in one process, --iters calls per timing); the baseline runs twice per round ("base-2").

    python tools/time_rwkv6_snap.py [--parent-lib PATH] [--out profiles/rwkv6_snap_time.txt]
"""
import argparse
import os
import sys

import timing
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rwkv_lm_ext_amd import _lib          # noqa: E402

bf = torch.bfloat16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warm", type=float, default=0.5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H = a.H
    C = 64 * H
    log = timing.Log()
    say = log.say

    lib = _lib.load()
    parent = lib
    if a.parent_lib:
        parent = timing.load_library(a.parent_lib, {"rwkv6_forward_varlen_bf16": _lib.SIGNATURES["rwkv6_forward_varlen_bf16"]},
                                     lacks=("rwkv6_forward_varlen_snap_bf16", "the snap call"))
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(0)
    p = lambda t: None if t is None else t.data_ptr()
    i32 = lambda x: torch.tensor(list(x), dtype=torch.int32, device="cuda")
    u = (torch.randn(H, 64, device="cuda", generator=g) * 0.3).to(bf)

    def batch(n_seq, length):
        total = n_seq * length
        r, k, v = (torch.randn(total, C, device="cuda", generator=g).mul_(0.5).to(bf) for _ in range(3))
        w = torch.exp(-torch.exp(torch.randn(total, C, device="cuda", generator=g) - 2.0)).contiguous()
        return dict(r=r, k=k, v=v, w=w, y=torch.empty(total, C, device="cuda", dtype=bf), cu=i32(range(0, total + 1, length)),
                    ws=torch.empty(lib.rwkv6_varlen_workspace_bytes(n_seq), dtype=torch.uint8, device="cuda"), n_seq=n_seq, length=length,
                    total=total)

    def pieces(d, n):
        """The batch as n batches of its sequences' consecutive n-ths, each packed on its own (how a caller cuts its prompts today)."""
        step = d["length"] // n
        out = []
        for i in range(n):
            rows = torch.cat([torch.arange(s * d["length"] + i * step, s * d["length"] + (i + 1) * step) for s in range(d["n_seq"])]).cuda()
            q = dict(d, length=step, total=d["n_seq"] * step, cu=i32(range(0, d["n_seq"] * step + 1, step)), rows=rows,
                     y=torch.empty(d["n_seq"] * step, C, device="cuda", dtype=bf))
            for x in ("r", "k", "v", "w"):
                q[x] = d[x][rows].contiguous()
            out.append(q)
        return out

    def bind(which, d, pool, slot, snap=None):
        args = (d["total"], d["n_seq"], d["length"], C, H, p(d["cu"]), p(slot), pool.shape[0], p(pool), p(d["r"]), p(d["k"]), p(d["v"]), p(d["w"]),
                p(u), p(d["y"]), p(d["ws"]), d["ws"].numel(), 0, stream)
        if snap is None:
            fn = which.rwkv6_forward_varlen_bf16
        else:
            slot_out, every, cu_snap, snap_slot = snap
            fn = which.rwkv6_forward_varlen_snap_bf16
            args += (p(slot_out), every, p(cu_snap), p(snap_slot), 0 if snap_slot is None else snap_slot.numel())
        return timing.bound(fn, *args)

    say(timing.device_header())
    where = "the parent commit's library" if a.parent_lib else "this library"
    say(f"bf16, H={H}, C={C}; baselines from {where}; {a.iters} calls per timing, {a.repeats} alternated repeats, {a.warm:.1f} s warm-up each")
    say()

    timed = lambda fn: timing.event_time(fn, a.iters) * 1e3                 # us per call (or per chain of calls)

    def race(title, new, base):
        for fn in (new, base):
            timing.warm(fn, seconds=a.warm)
        res = timing.alternate({"snap": new, "base": base, "base-2": base}, timed, a.repeats)
        for n, xs in res.items():
            say(f"  {n:8s} us: " + timing.values_and_stats(xs, 8, 1))
        m = {n: timing.median(xs) for n, xs in res.items()}
        lo, hi = min(res["base"] + res["base-2"]), max(res["base"] + res["base-2"])
        say(f"  snap / base = {m['snap'] / m['base']:.3f} ({m['snap'] - m['base']:+.1f} us, {100 * (m['snap'] / m['base'] - 1):+.1f} %); "
            f"base against itself: {m['base-2'] / m['base']:.3f}, range [{lo:.1f}, {hi:.1f}] us; "
            f"{'ranges do not overlap' if timing.apart(res['snap'], (lo, hi)) else 'ranges overlap'}")
        say()
        return m

    # ---- (a), (b): 8 prompts of 1024 tokens, a snapshot every 256
    n_seq, length, every = 8, 1024, 256
    n_snap = n_seq * (length // every)
    d = batch(n_seq, length)
    chain = pieces(d, length // every)
    start = torch.randn(n_seq + n_snap, H, 64, 64, device="cuda", generator=g) * 0.5
    pool_new, pool_base, pool_one = start.clone(), start.clone(), start.clone()
    snap_args = (None, every, i32(range(0, n_snap + 1, length // every)), i32(range(n_seq, n_seq + n_snap)))
    new = bind(lib, d, pool_new, None, snap_args)
    links = [bind(parent, q, pool_base, None) for q in chain]
    one = bind(parent, d, pool_one, None)

    def run_chain():
        for fn in links:
            fn()

    new()
    want = start.clone()
    y_chain = torch.empty_like(d["y"])
    for i, (fn, q) in enumerate(zip(links, chain)):
        fn()
        want[n_seq + i:n_seq + n_snap:length // every] = pool_base[:n_seq]   # snapshot i of sequence s lives in slot n_seq + 4 s + i
        y_chain[q["rows"]] = q["y"]
    want[:n_seq] = pool_base[:n_seq]
    y_new = d["y"].clone()
    one()
    torch.cuda.synchronize()
    same_b = bool(torch.equal(y_new, d["y"]) and torch.equal(pool_new[:n_seq], pool_one[:n_seq]))     # (before the timed calls move the pools on)
    say(f"(a) 8 x 1024, a snapshot every 256: y, final states and the 32 snapshots of the snap call == the chain of four calls, bit for bit: "
        f"{bool(torch.equal(y_new, y_chain) and torch.equal(pool_new, want))}")
    ma = race("(a)", new, run_chain)
    say(f"(b) the same snap call against the single call without snapshots: y and final states equal, bit for bit: "
        f"{same_b}")
    mb = race("(b)", new, one)

    # ---- (c): 8 sequences of 512 tokens from cached slots 0..7 into slots 8..15
    e = batch(8, 512)
    start_c = torch.randn(16, H, 64, 64, device="cuda", generator=g) * 0.5
    pool_cn, pool_cb = start_c.clone(), start_c.clone()
    src, dst = i32(range(8)), i32(range(8, 16))
    new_c = bind(lib, e, pool_cn, src, (dst, 0, None, None))
    base_call = bind(parent, e, pool_cb, dst)

    def copy_then_call():
        pool_cb[8:].copy_(pool_cb[:8])
        base_call()

    new_c()
    y_new = e["y"].clone()
    copy_then_call()
    torch.cuda.synchronize()
    say(f"(c) 8 x 512 from slots 0..7 into slots 8..15: y and the pool of the snap call == copy + in-place call, bit for bit: "
        f"{bool(torch.equal(y_new, e['y']) and torch.equal(pool_cn, pool_cb))}")
    mc = race("(c)", new_c, copy_then_call)

    stores = n_snap * H * 4096 * 4
    say(f"(a) one snap call is {ma['base'] / ma['snap']:.2f}x the speed of the chain of four calls"
        f" -> {'the snap call is faster' if ma['snap'] < ma['base'] else 'THE SNAP CALL IS NOT FASTER THAN THE CHAIN'}")
    say(f"(b) the snapshots cost {mb['snap'] - mb['base']:+.1f} us ({100 * (mb['snap'] / mb['base'] - 1):+.1f} %) for {stores / 2**20:.0f} MiB of stores: "
        f"{stores / max(mb['snap'] - mb['base'], 1e-3) / 1e6:.2f} TB/s if the difference were the stores alone")
    say(f"(c) one call with output slots against copy + call: {mc['snap'] - mc['base']:+.1f} us ({100 * (mc['snap'] / mc['base'] - 1):+.1f} %)")
    log.write(a.out)


if __name__ == "__main__":
    main()
