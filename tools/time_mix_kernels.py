#!/usr/bin/env python3
"""Time the elementwise HIP kernels of csrc/wkv6_mix.hip at B x T = 48 x 512 rows, C = 2048 (BASELINE configs[2] layer shape)
and report their algorithmic HBM bandwidth:   python tools/time_mix_kernels.py

The token shift in every form the library has -- dense, dense under a reversal map (rev_n), packed (48 sequences of 512), packed under a
map, and the slot-pool pair ddlerp_slots + shift_keep (256 slots) -- for the three (NS, m) pairs the model uses, then gn_gate.
RWKV_AMD_LIB names another build of the library (rwkv_lm_ext_amd/_lib.py): the same script then times that one."""
import os
import sys

import timing
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rwkv_lm_ext_amd import mix_op                                 # noqa: E402

dev = torch.device("cuda", 0)
B, T, C, H = 48, 512, 2048, 32
N_SLOTS = 256
bf = torch.bfloat16
g = torch.Generator(device=dev).manual_seed(0)
rnd = lambda *s: torch.randn(*s, device=dev, generator=g).to(bf)
i32 = lambda v: torch.as_tensor(v, dtype=torch.int32).to(dev)
tc = B * T * C


timeit = lambda fn: timing.one_shot(fn, 50, 10) * 1e3     # us
rows = []
cu = i32([T * s for s in range(B + 1)])
rev_n = torch.randint(0, T + 1, (B,), device=dev, generator=g).to(torch.int32)
slots = torch.randperm(N_SLOTS, device=dev, generator=g)[:B].to(torch.int32)
pool = rnd(N_SLOTS, C)
for ns, has_m in ((5, True), (1, False), (2, False)):
    x = rnd(B, T, C).requires_grad_(True)
    maa = rnd(ns, C).requires_grad_(True)
    m = rnd(ns, B, T, C).requires_grad_(True) if has_m else None
    dout = rnd(ns, B, T, C)
    xp, mp = x.detach().view(1, B * T, C).requires_grad_(True), None if m is None else m.detach().view(ns, 1, B * T, C).requires_grad_(True)
    bytes_f = 2 + 2 * ns + (2 * ns if has_m else 0)                  # x, out, m
    bytes_b = 2 + 2 * ns + 2 + (4 * ns if has_m else 0)              # x, dout, dx, m + dm
    bytes_far = bytes_b + 2 * ns + (2 * ns if has_m else 0)          # under a map the neighbour's dout and m are read a second time
    for form, xs, ms, kw, bb in (("dense", x, m, {}, bytes_b), ("dense rev_n", x, m, dict(rev_n=rev_n), bytes_far),
                                 ("packed", xp, mp, dict(cu_seqlens=cu), bytes_b),
                                 ("packed rev_n", xp, mp, dict(cu_seqlens=cu, rev_n=rev_n), bytes_far)):
        fwd = lambda: mix_op.ddlerp(xs, maa, ms, **kw)
        out = fwd()
        def bwd():
            xs.grad = maa.grad = None
            if ms is not None:
                ms.grad = None
            out.backward(dout.view_as(out), retain_graph=True)
        rows.append((f"ddlerp fwd NS={ns} {form}", timeit(fwd), bytes_f))
        rows.append((f"ddlerp bwd NS={ns} {form} (+ torch partial sums)", timeit(bwd), bb))
        del out
    with torch.no_grad():
        xd, md = xp.detach(), None if mp is None else mp.detach()
        rows.append((f"ddlerp_slots fwd NS={ns}", timeit(lambda: mix_op.ddlerp_slots(xd, maa.detach(), md, pool, slots, cu)), bytes_f))
with torch.no_grad():
    xk = rnd(1, B * T, C)
    us = timeit(lambda: mix_op.shift_keep(xk, cu, T, pool, slots))
    print(f"{'shift_keep (48 last tokens -> 256-slot pool)':52s} {us:8.1f} us   (copies {B} rows of {C}: a launch, not a bandwidth figure)")
y, gt = rnd(B * T, C).requires_grad_(True), rnd(B * T, C).requires_grad_(True)
gamma, beta = rnd(C).requires_grad_(True), rnd(C).requires_grad_(True)
dout = rnd(B * T, C)
out = mix_op.group_norm_gate(y, gt, gamma, beta, H, 64e-5)
rows.append(("gn_gate fwd", timeit(lambda: mix_op.group_norm_gate(y, gt, gamma, beta, H, 64e-5)), 6))
def gbwd():
    y.grad = gt.grad = gamma.grad = beta.grad = None
    out.backward(dout, retain_graph=True)
rows.append(("gn_gate bwd (+ torch partial sums)", timeit(gbwd), 10))
print(f"# B x T = {B} x {T}, C = {C}: {tc / 1e6:.1f} M token-channels; HIP-event time per autograd call (kernel + allocations + the small torch reductions)")
for name, us, b in rows:
    print(f"{name:52s} {us:8.1f} us   {b:3d} B/tc   {b * tc / us / 1e6:5.2f} TB/s  = {100 * b * tc / us / 1e6 / 8:4.1f} % of 8 TB/s")
