"""How far an fp32-accumulating chain may lie from the fp64 restatement of the low-rank time-mix inputs (tests/lowrank_common.py), on the
CPU: the measurement behind K_BOUND of tests/test_lowrank_gpu.py.

On exactly the inputs of the GPU parity cases -- lc.TMIX_CASES: every width and row count under the packed batch lc.CU with the slots
lc.SLOTS, and the many-tiles case under lc.many_batch(); lc.DECAY_NC_CASES: the decay with dim_att N != C -- the chain (lerp, W1, tanh,
W2, lerp; and the decay on the restatement's xw) is emulated with its contractions summed in fp32 in three orders -- torch's own, K
reversed, K in 4 interleaved chunks -- and compared with the restatement: the share of elements whose bits differ, and the largest
|diff| / (ulp(b) + 1 * extra) among them (the bound at k = 1).  K_BOUND is twice the largest ratio seen, rounded up to a power of two.
tests/test_lowrank_cpu.py asserts the same figures (ratio <= K_BOUND / 2, share <= CAP) on every run of the suite.

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
    worst = {"out": 0.0, "w": 0.0, "share": 0.0}
    print("fp32-accumulating emulations of the chain against the fp64 restatement (CPU, torch %s)" % torch.__version__)
    print("inputs: those of the GPU parity cases (tests/lowrank_common.py: make_inputs, TMIX_CASES -- WIDTHS x ROWS under the batch CU with "
          "the slots SLOTS, and MANY_T rows under many_batch() -- and DECAY_NC_CASES -- DECAY_CASES x ROWS)")
    for scale in (0.25, 2.0):
        if scale != 0.25:
            print("-- W2 and D2 scaled by %.1f instead of 0.25 (reported, not part of K_BOUND)" % scale)
        print("%-5s %-4s %-4s %-5s %-26s %12s %10s %12s %10s" % ("C", "D", "Dd", "rows", "order", "out differ %", "out ratio", "w differ %", "w ratio"))
        for C, D, Dd, rows in lc.TMIX_CASES:
            case = lc.tmix_case(C, D, Dd, rows, w2_scale=scale)
            for name, mm in lc.ORDERS.items():
                so, ro, sw, rw = lc.emulate_tmix(case, mm)
                print("%-5d %-4d %-4d %-5d %-26s %12.4f %10.3f %12.4f %10.3f" % (C, D, Dd, rows, name, so * 100, ro, sw * 100, rw))
                if scale == 0.25:
                    worst["out"], worst["w"], worst["share"] = max(worst["out"], ro), max(worst["w"], rw), max(worst["share"], so, sw)
        print("decay_lowrank with dim_att N != C (xw = the x of make_inputs)")
        print("%-5s %-4s %-4s %-5s %-26s %12s %10s" % ("C", "N", "Dd", "rows", "order", "w differ %", "w ratio"))
        for C, N, Dd, rows in lc.DECAY_NC_CASES:
            case = lc.decay_case(C, N, Dd, rows, w2_scale=scale)
            for name, mm in lc.ORDERS.items():
                sw, rw = lc.emulate_decay(case, mm)
                print("%-5d %-4d %-4d %-5d %-26s %12.4f %10.3f" % (C, N, Dd, rows, name, sw * 100, rw))
                if scale == 0.25:
                    worst["w"], worst["share"] = max(worst["w"], rw), max(worst["share"], sw)
    top = max(worst["out"], worst["w"])
    k = 2.0 ** math.ceil(math.log2(2 * top)) if top > 0 else 1.0
    print("largest ratio to the bound at k = 1: out %.3f, w %.3f" % (worst["out"], worst["w"]))
    print("largest share of differing elements: %.4f %% (CAP = %g %%)" % (worst["share"] * 100, lc.CAP * 100))
    print("K_BOUND = 2 * %.3f rounded up to a power of two = %g" % (top, k))


if __name__ == "__main__":
    main()
