"""How far an fp32-accumulating chain may lie from the fp64 restatement of the low-rank time-mix inputs (tests/lowrank_common.py), on the
CPU: the measurement behind K_BOUND of tests/test_lowrank_gpu.py.

On exactly the inputs of the GPU parity cases -- every width and row count, the packed batch lc.CU with the slots lc.SLOTS -- the chain (lerp, W1, tanh, W2, lerp; and the decay on the restatement's xw) is
emulated with its contractions summed in fp32 in three orders -- torch's own, K reversed, K in 4 interleaved chunks -- and compared with
the restatement: the share of elements whose bits differ, and the largest |diff| / (ulp(b) + 1 * extra) among them (the bound at k = 1).
K_BOUND is twice the largest ratio seen, rounded up to a power of two.

    python tools/lowrank_parity.py > profiles/lowrank_parity.txt
"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import lowrank_common as lc                                         # noqa: E402


def main():
    torch.set_num_threads(min(8, torch.get_num_threads()))
    worst = {"out": 0.0, "w": 0.0}
    print("fp32-accumulating emulations of the chain against the fp64 restatement (CPU, torch %s)" % torch.__version__)
    print("inputs: those of the GPU parity cases (tests/lowrank_common.py: make_inputs, WIDTHS, ROWS, the batch CU with the slots SLOTS)")
    print("%-5s %-4s %-4s %-5s %-26s %12s %10s %12s %10s" % ("C", "D", "Dd", "rows", "order", "out differ %", "out ratio", "w differ %", "w ratio"))
    for scale in (0.25, 2.0):
        if scale != 0.25:
            print("-- W2 and D2 scaled by %.1f instead of 0.25 (reported, not part of K_BOUND)" % scale)
        for C, D, Dd in lc.WIDTHS:
            for rows in lc.ROWS:
                p = lc.make_inputs(C, D, Dd, rows, w2_scale=scale)
                xp = lc.token_in_front(p["x"], lc.cu_of(rows), p["front"], list(lc.SLOTS))
                out, corr, d = lc.restate_tmix(p, xp)
                xw = out[0].to(torch.bfloat16)
                w, corr_w = lc.restate_decay(p, xw)
                for name, mm in lc.ORDERS.items():
                    got, _, _ = lc.restate_tmix(p, xp, matmul=mm)
                    so, ro = lc.compare(got, out, lc.bound_out(out, corr, d, 1.0))
                    gw, _ = lc.restate_decay(p, xw, matmul=mm)
                    sw, rw = lc.compare(gw, w, lc.bound_w(w, corr_w, 1.0))
                    print("%-5d %-4d %-4d %-5d %-26s %12.4f %10.3f %12.4f %10.3f" % (C, D, Dd, rows, name, so * 100, ro, sw * 100, rw))
                    if scale == 0.25:
                        worst["out"], worst["w"] = max(worst["out"], ro), max(worst["w"], rw)
    top = max(worst.values())
    k = 2.0 ** math.ceil(math.log2(2 * top)) if top > 0 else 1.0
    print("largest ratio to the bound at k = 1: out %.3f, w %.3f" % (worst["out"], worst["w"]))
    print("K_BOUND = 2 * %.3f rounded up to a power of two = %g" % (top, k))


if __name__ == "__main__":
    main()
