"""What 0 / 1 / 2 / 3 device event records per fwd+bwd step cost the stream: host time per step over 200 steps (bench.py uses two per step).
The events are what is measured here, so the loop is this tool's own; only the warm-up is the shared one (tools/timing.py)."""
import os
import sys
import time

import timing
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                                       # noqa: E402

dev = torch.device('cuda', 0)
fwd, bwd = bench.build_workload('wkv6', dev)[:2]
fwd(); bwd(); torch.cuda.synchronize()
def timed(n, mode):
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(n)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        if mode >= 1: evs[i][0].record()
        fwd()
        if mode >= 2: evs[i][1].record()
        bwd()
        if mode >= 3: evs[i][2].record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n
bench.prewarm_until_steady(fwd, bwd)
for rep in range(3):
    for mode in (0, 1, 2, 3):
        timing.warm(lambda: (fwd(), bwd()), calls=50, sync=None)
        print(rep, 'events per step', mode, 'ms per step %.4f' % timed(200, mode), flush=True)
