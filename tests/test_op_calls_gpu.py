"""The library calls of the operator layer, pinned without running a kernel: every wrapper of wkv6_op and every op of mix_op is called once
per materially different route with `_lib.load` patched to return a recorder, and the recorded (symbol, arguments) lists must equal
tests/op_calls_expected.json record by record.  A pointer in the wrong position of a ctypes argument list shows here as a changed name,
before anything is launched.

Normalised arguments: the data_ptr() of a named input -> its name; the current stream's handle -> "stream" (the calls run under a
non-default stream, so the handle is not 0); any other integer above 1 << 32 -> "fresh" (a tensor the wrapper allocated); None, small
integers, floats and flag words as they are; a SeqSet * 2 array field by field under the same rules.  The recorder answers 4096 to every
*_bytes symbol and 0 to every other one.  No library code runs: only torch.empty / torch.zeros allocations (and the few eager torch
kernels of the wrappers' own epilogues) touch the device.

Shapes: B = 2, T = 8, H = 2, C = 128; packed: total_T = 8, cu_seqlens = [0, 3, 8]; LoRA: K = N = 64, R = 8, 2 adapters.

    python tests/test_op_calls_gpu.py > tests/op_calls_expected.json      # prints the records of the tree it is run in

The second test holds the refusals that need a GPU tensor to be reached (dtype after is_cuda, contiguity, shape, C != H*64, an int array
on another device): each raises before anything is launched, and before the library is loaded where it did so when the table was written."""
import ctypes
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EXPECTED = os.path.join(HERE, "op_calls_expected.json")
B, T, H, C, N = 2, 8, 2, 128, 64
TOTAL, CU, NSEQ = 8, (0, 3, 8), 2


class Recorder:
    """Stands in for the loaded library: every attribute is a function that records its normalised call."""

    def __init__(self, torch):
        self._torch, self.records, self.names, self.keep, self.label = torch, [], {}, [], None

    def norm(self, a):
        if isinstance(a, ctypes.Array):                                       # SeqSet * 2
            return [{f: self.norm(getattr(e, f)) for f, _ in e._fields_} for e in a]
        if isinstance(a, bool) or not isinstance(a, int):
            return a
        if a in self.names:
            return self.names[a]
        if a == self._torch.cuda.current_stream().cuda_stream:
            return "stream"
        return "fresh" if a > 1 << 32 else a

    def __getattr__(self, symbol):
        if symbol.startswith("__"):
            raise AttributeError(symbol)

        def fn(*args):
            self.records.append([self.label, symbol, [self.norm(a) for a in args]])
            return 4096 if symbol.endswith("_bytes") else 0
        return fn

    def t(self, name, shape, dtype):
        x = self._torch.zeros(shape, dtype=dtype, device="cuda")
        self.names[x.data_ptr()] = name
        self.keep.append(x)                     # named inputs live to the end: no two of them share an address
        return x

    def ints(self, name, values):
        x = self._torch.tensor(list(values), dtype=self._torch.int32, device="cuda")
        self.names[x.data_ptr()] = name
        self.keep.append(x)
        return x


def record(torch, rec):
    """Call every route; rec.records is the result."""
    from rwkv_lm_ext_amd import mix_op, wkv6_op as op
    bf, f16, f32, u8 = torch.bfloat16, torch.float16, torch.float32, torch.uint8
    t, ints = rec.t, rec.ints

    def route(label, fn, *args, **kw):
        rec.label = label
        return fn(*args, **kw)

    def dense(io):          # r, k, v, w, u, gy + caller-side outputs, named by role
        d = {n: t(n, (B, T, C), io) for n in ("r", "k", "v", "w", "gy", "y", "gr", "gk", "gv", "gw")}
        d.update(u=t("u", (H, N), io), ew=t("w", (B, T, C), f32), gu=t("gu", (B, C), io))
        return d

    def packed(io):
        d = {n: t(n, (TOTAL, C), io) for n in ("r", "k", "v", "w", "gy", "y", "gr", "gk", "gv", "gw")}
        d.update(u=t("u", (H, N), io), ew=t("w", (TOTAL, C), f32), gu=t("gu", (NSEQ, C), f32))
        return d

    D, P = {io: dense(io) for io in (bf, f16, f32)}, {io: packed(io) for io in (bf, f16, f32)}
    d, p = D[bf], P[bf]
    rkv = lambda q: (q["r"], q["k"], q["v"])
    grads = lambda q: (q["gy"], q["gr"], q["gk"], q["gv"], q["gw"])
    cu = ints("cu_seqlens", CU)
    ws = lambda name="ws": t(name, (4096,), u8)

    # ---- the six module objects
    route("wkv6_cuda.forward", op.wkv6_cuda.forward, B, T, C, H, *rkv(d), d["ew"], d["u"], d["y"])
    route("wkv6_cuda.backward", op.wkv6_cuda.backward, B, T, C, H, *rkv(d), d["ew"], d["u"], *grads(d), d["gu"])
    mask = t("mask", (B, T), torch.int32)
    route("wkv6_bi_cuda.forward", op.wkv6_bi_cuda.forward, B, T, C, H, mask, *rkv(d), d["ew"], d["u"], d["y"])
    route("wkv6_bi_cuda.backward", op.wkv6_bi_cuda.backward, B, T, C, H, mask, *rkv(d), d["ew"], d["u"], *grads(d), d["gu"])
    s3, s4, gs = t("s", (H, N, N), bf), t("s", (B, H, N, N), bf), t("gs", (B, H, N, N), bf)
    for mod, name, s in ((op.wkv6state_cuda, "wkv6state_cuda", s3), (op.wkv6infctx_cuda, "wkv6infctx_cuda", s4)):
        route(name + ".forward", mod.forward, B, T, C, H, *rkv(d), d["w"], d["u"], s, d["y"])
        route(name + ".backward", mod.backward, B, T, C, H, *rkv(d), d["w"], d["u"], s, *grads(d), d["gu"], gs)
    w5, ww5 = t("w", (H, N), f32), t("ww", (H, N), f32)
    route("wkv5.forward", op.wkv5.forward, B, T, C, H, *rkv(d), w5, d["u"], d["y"])
    route("wkv5.backward", op.wkv5.backward, B, T, C, H, *rkv(d), w5, ww5, d["u"], d["gy"], d["gr"], d["gk"], d["gv"],
          t("gw", (B, C), bf), d["gu"])
    state = t("state", (B, H, N, N), f32)
    for io, sfx in ((bf, "bf16"), (f16, "fp16"), (f32, "fp32")):
        q = D[io]
        route("rwkv6.forward_" + sfx, getattr(op.rwkv6, "forward_" + sfx), B, T, C, H, state, *rkv(q), q["ew"], q["u"], q["y"])

    # ---- rwkv6.forward_varlen_*: all nine
    pool, slot, slot_out = t("state_pool", (4, H, N, N), f32), ints("state_slot", (1, 0)), ints("state_slot_out", (2, 3))
    cu_snap, snap_slot = ints("cu_snap", (0, 0, 1)), ints("snap_slot", (3,))
    for io, sfx in ((bf, "bf16"), (f16, "fp16"), (f32, "fp32")):
        q = P[io]
        plain, snap = getattr(op.rwkv6, "forward_varlen_" + sfx), getattr(op.rwkv6, "forward_varlen_snap_" + sfx)
        a = (*rkv(q), q["ew"], q["u"], q["y"], cu, 8)
        route(f"rwkv6.forward_varlen_{sfx} plain", plain, TOTAL, C, H, pool, None, *a)
        route(f"rwkv6.forward_varlen_{sfx} slot scan ws", plain, TOTAL, C, H, pool, slot, *a, "scan", ws())
        route(f"rwkv6.forward_varlen_{sfx} slot_out", plain, TOTAL, C, H, pool, slot, *a, state_slot_out=slot_out)
        route(f"rwkv6.forward_varlen_{sfx} snap", plain, TOTAL, C, H, pool, slot, *a, None, None, slot_out, 64, cu_snap, snap_slot)
        route(f"rwkv6.forward_varlen_snap_{sfx} defaults", snap, TOTAL, C, H, pool, None, None, *a, 0, None, None)
        route(f"rwkv6.forward_varlen_snap_{sfx} all", snap, TOTAL, C, H, pool, slot, slot_out, *a, 64, cu_snap, snap_slot)
        route(f"torch.ops.rwkv6.forward_varlen_{sfx}", getattr(torch.ops.rwkv6, "forward_varlen_" + sfx), TOTAL, C, H, pool, slot, *a)
        route(f"torch.ops.rwkv6.forward_varlen_snap_{sfx}", getattr(torch.ops.rwkv6, "forward_varlen_snap_" + sfx), TOTAL, C, H, pool,
              None, slot_out, *a, 0, None, None)
    a = (*rkv(p), p["ew"], p["u"], p["y"], cu, 8)
    route("rwkv6.forward_varlen_bf16 seg_len", op.rwkv6.forward_varlen_bf16, TOTAL, C, H, pool, slot, *a, seg_len=64)
    route("rwkv6.forward_varlen_bf16 seg_len snap ws", op.rwkv6.forward_varlen_bf16, TOTAL, C, H, pool, slot, *a, None, ws(), slot_out, 64,
          cu_snap, snap_slot, 64)
    route("rwkv6.forward_varlen_split_bf16 seg_len 0", op.rwkv6.forward_varlen_split_bf16, TOTAL, C, H, pool, None, None, *a, 0, None,
          None, 0)
    route("rwkv6.forward_varlen_split_bf16 all ws", op.rwkv6.forward_varlen_split_bf16, TOTAL, C, H, pool, slot, slot_out, *a, 64, cu_snap,
          snap_slot, 64, ws())
    route("torch.ops.rwkv6.forward_varlen_split_bf16", torch.ops.rwkv6.forward_varlen_split_bf16, TOTAL, C, H, pool, slot, None, *a, 0, None,
          None, 64)

    # ---- workspaces and small things
    route("new_checkpoint", op.new_checkpoint, B, T, C, H, "cuda")
    route("new_varlen_workspace", op.new_varlen_workspace, TOTAL, NSEQ, C, H, "cuda")
    route("new_rwkv6_varlen_workspace", op.new_rwkv6_varlen_workspace, NSEQ, "cuda")
    route("new_rwkv6_varlen_split_workspace", op.new_rwkv6_varlen_split_workspace, TOTAL, NSEQ, 64, C, H, "cuda")
    route("bi_new_workspace", op.bi_new_workspace, B, T, C, H, "cuda")
    route("bi_new_kept", op.bi_new_kept, B, T, C, H, "cuda")
    route("selftest", op.selftest)
    route("pass_marker", op.pass_marker)

    # ---- forward_ex / forward_gn_ex / backward_ex
    q32 = D[f32]
    s0_3, s0_4, s_out = t("s0", (H, N, N), bf), t("s0", (B, H, N, N), bf), t("s_out", (B, H, N, N), bf)
    ckpt = ws("ckpt")
    x5 = lambda q: (*rkv(q), q["w"], q["u"])
    route("forward_ex plain", op.forward_ex, *x5(d), H)
    route("forward_ex ckpt y", op.forward_ex, *x5(d), H, y=d["y"], ckpt=ckpt)
    route("forward_ex s0 3-d", op.forward_ex, *x5(d), H, s0=s0_3)
    route("forward_ex s0 4-d s_out", op.forward_ex, *x5(d), H, s0_4, s_out)
    route("forward_ex w_is_ew", op.forward_ex, *rkv(d), d["ew"], d["u"], H, w_is_ew=True)
    route("forward_ex scan", op.forward_ex, *x5(d), H, algo="scan")
    route("forward_ex fp32", op.forward_ex, *x5(q32), H)
    route("forward_ex fp32 w_is_ew scan s0 ckpt", op.forward_ex, *rkv(q32), q32["ew"], q32["u"], H, t("s0", (B, H, N, N), f32), None, True,
          None, "scan", ckpt)
    gate, gamma, beta = t("gate", (B, T, C), bf), t("gamma", (C,), bf), t("beta", (C,), bf)
    route("forward_gn_ex", op.forward_gn_ex, *x5(d), H, gate, gamma, beta, 64e-5)
    route("forward_gn_ex ckpt no y no stats", op.forward_gn_ex, *x5(d), H, gate, gamma, beta, 1e-5, ckpt, False, False)
    x6 = lambda q: (*x5(q), q["gy"])
    route("backward_ex plain", op.backward_ex, *x6(d), H)
    route("backward_ex ckpt", op.backward_ex, *x6(d), H, ckpt=ckpt)
    route("backward_ex want_gs s0 4-d", op.backward_ex, *x6(d), H, s0_4, False, True)
    route("backward_ex s0 3-d w_is_ew scan", op.backward_ex, *rkv(d), d["ew"], d["u"], d["gy"], H, s0_3, True, False, "scan")
    route("backward_ex fp32", op.backward_ex, *x6(q32), H)
    route("backward_ex fp32 scan ckpt", op.backward_ex, *x6(q32), H, algo="scan", ckpt=ckpt)      # ckpt alone sets CKPT_VALID here

    # ---- packed
    p32 = P[f32]
    ps0_3, ps0_4, ps_out = t("s0", (H, N, N), bf), t("s0", (NSEQ, H, N, N), bf), t("s_out", (NSEQ, H, N, N), bf)
    route("forward_varlen_ex plain", op.forward_varlen_ex, *x5(p), H, cu, 5)
    route("forward_varlen_ex s0 4-d s_out y ws", op.forward_varlen_ex, *x5(p), H, cu, 5, ps0_4, ps_out, False, p["y"], None, ws())
    route("forward_varlen_ex s0 3-d w_is_ew scan", op.forward_varlen_ex, *rkv(p), p["ew"], p["u"], H, cu, 5, ps0_3, w_is_ew=True, algo="scan")
    route("forward_varlen_ex fp32", op.forward_varlen_ex, *x5(p32), H, cu, 5)
    route("backward_varlen_ex plain", op.backward_varlen_ex, *x6(p), H, cu, 5)
    route("backward_varlen_ex ws ckpt_valid", op.backward_varlen_ex, *x6(p), H, cu, 5, ws=ws(), ckpt_valid=True)
    route("backward_varlen_ex ws only", op.backward_varlen_ex, *x6(p), H, cu, 5, ws=ws())
    route("backward_varlen_ex ckpt_valid scan want_gs s0", op.backward_varlen_ex, *x6(p), H, cu, 5, ps0_4, False, True, "scan", ws(), True)
    route("backward_varlen_ex ckpt_valid fp32", op.backward_varlen_ex, *x6(p32), H, cu, 5, ws=ws(), ckpt_valid=True)
    route("backward_varlen_ex w_is_ew", op.backward_varlen_ex, *rkv(p), p["ew"], p["u"], p["gy"], H, cu, 5, w_is_ew=True)
    route("torch.ops.wkv6.forward_varlen", torch.ops.wkv6.forward_varlen, TOTAL, C, H, *x5(p), cu, 5, p["y"])
    route("torch.ops.wkv6.backward_varlen", torch.ops.wkv6.backward_varlen, TOTAL, C, H, *x5(p), cu, 5, *grads(p), p["gu"])

    # ---- wkv5
    hn = lambda io: (t("w", (H, N), io), t("u", (H, N), io))
    route("wkv5_forward_ex", op.wkv5_forward_ex, *rkv(d), *hn(bf), H)
    route("wkv5_forward_ex fp32 y", op.wkv5_forward_ex, *rkv(q32), *hn(f32), H, q32["y"])
    route("wkv5_backward_ex", op.wkv5_backward_ex, *rkv(d), *hn(bf), d["gy"], H)
    route("wkv5_backward_ex fp32", op.wkv5_backward_ex, *rkv(q32), *hn(f32), q32["gy"], H)

    # ---- reversal maps
    rev_b, rev_s = ints("rev_n", (3, 8)), ints("rev_n", (2, 5))
    route("forward_rev_ex", op.forward_rev_ex, *x5(d), H, rev_b, op.REV_K | op.REV_Y)
    route("forward_rev_ex y ckpt scan", op.forward_rev_ex, *x5(d), H, rev_b, op.REV_ALL, d["y"], ckpt, "scan")
    route("forward_rev_ex fp32", op.forward_rev_ex, *x5(q32), H, rev_b, op.REV_R)
    route("backward_rev_ex", op.backward_rev_ex, *x6(d), H, rev_b, op.REV_K | op.REV_Y)
    route("backward_rev_ex ckpt", op.backward_rev_ex, *x6(d), H, rev_b, op.REV_ALL, ckpt)
    route("backward_rev_ex ckpt scan", op.backward_rev_ex, *x6(d), H, rev_b, op.REV_ALL, ckpt, "scan")
    route("backward_rev_ex ckpt fp32", op.backward_rev_ex, *x6(q32), H, rev_b, op.REV_V, ckpt)
    route("forward_varlen_rev_ex", op.forward_varlen_rev_ex, *x5(p), H, cu, 5, rev_s, op.REV_K | op.REV_Y)
    route("forward_varlen_rev_ex no map y scan ws", op.forward_varlen_rev_ex, *x5(p), H, cu, 5, None, 0, p["y"], "scan", ws())
    route("forward_varlen_rev_ex w_is_ew fp32", op.forward_varlen_rev_ex, *rkv(p32), p32["ew"], p32["u"], H, cu, 5, rev_s, op.REV_W,
          w_is_ew=True)
    route("backward_varlen_rev_ex", op.backward_varlen_rev_ex, *x6(p), H, cu, 5, rev_s, op.REV_K | op.REV_Y)
    route("backward_varlen_rev_ex no map ws ckpt_valid", op.backward_varlen_rev_ex, *x6(p), H, cu, 5, None, 0, None, ws(), True)
    route("backward_varlen_rev_ex scan ws ckpt_valid", op.backward_varlen_rev_ex, *x6(p), H, cu, 5, rev_s, op.REV_ALL, "scan", ws(), True)
    route("backward_varlen_rev_ex fp32 ws ckpt_valid w_is_ew", op.backward_varlen_rev_ex, *rkv(p32), p32["ew"], p32["u"], p32["gy"], H, cu, 5,
          rev_s, op.REV_R, None, ws(), True, True)

    # ---- pair launches
    def sets(shape, rev, bwd, given):
        out = []
        for i in range(2):
            q = {n: t(f"{n}{i}", shape, bf) for n in ("r", "k", "v", "w") + (("gy",) if bwd else ())}
            if given or bwd:
                q["ckpt"] = ws(f"ckpt{i}")
            if given and not bwd:
                q["y"] = t(f"y{i}", shape, bf)
            if i == 1 and rev is not None:
                q["rev_n"], q["rev_mask"] = rev, op.REV_ALL
            if i == 0 and given:
                q["rev_mask"] = op.REV_K             # without rev_n: the mask does not reach the library
            out.append(q)
        return out

    route("forward_pair_ex", op.forward_pair_ex, H, d["u"], sets((B, T, C), None, False, False))
    route("forward_pair_ex y ckpt rev", op.forward_pair_ex, H, d["u"], sets((B, T, C), rev_b, False, True))
    route("backward_pair_ex", op.backward_pair_ex, H, d["u"], sets((B, T, C), None, True, False))
    route("backward_pair_ex rev", op.backward_pair_ex, H, d["u"], sets((B, T, C), rev_b, True, True))
    route("forward_varlen_pair_ex", op.forward_varlen_pair_ex, H, p["u"], sets((TOTAL, C), None, False, False), cu, 5)
    route("forward_varlen_pair_ex y ckpt rev", op.forward_varlen_pair_ex, H, p["u"], sets((TOTAL, C), rev_s, False, True), cu, 5)
    route("backward_varlen_pair_ex", op.backward_varlen_pair_ex, H, p["u"], sets((TOTAL, C), None, True, False), cu, 5)
    route("backward_varlen_pair_ex rev", op.backward_varlen_pair_ex, H, p["u"], sets((TOTAL, C), rev_s, True, True), cu, 5)

    # ---- wkv6_bi
    lens = ints("lens", (8, 5))
    route("bi_forward_ex mask", op.bi_forward_ex, mask, *x5(d), H)
    route("bi_forward_ex lens ws", op.bi_forward_ex, None, *x5(d), H, ws=ws(), lens=lens)
    route("bi_forward_ex mask w_is_ew scan", op.bi_forward_ex, mask, *rkv(d), d["ew"], d["u"], H, True, "scan")
    route("bi_forward_ex lens fp32 ws", op.bi_forward_ex, None, *x5(q32), H, ws=ws(), lens=lens)
    route("bi_backward_ex mask", op.bi_backward_ex, mask, *x6(d), H)
    route("bi_backward_ex lens ws", op.bi_backward_ex, None, *x6(d), H, ws=ws(), lens=lens)
    route("bi_backward_ex mask w_is_ew scan ws", op.bi_backward_ex, mask, *rkv(d), d["ew"], d["u"], d["gy"], H, True, "scan", ws())
    route("bi_backward_ex lens fp32 ws", op.bi_backward_ex, None, *x6(q32), H, ws=ws(), lens=lens)
    route("bi_backward_ex mask fp32", op.bi_backward_ex, mask, *x6(q32), H)

    # ---- mix_op: ddlerp on its four routes, forward and backward through autograd
    NS = 5

    def leaf(name, shape):
        return t(name, shape, bf).requires_grad_(True)

    def ddlerp(label, xshape, s0shape, with_m, **kw):
        x, maa = leaf("x", xshape), leaf("maa", (NS if with_m else 1, 1, 1, C))
        m = leaf("m", (NS,) + xshape) if with_m else None
        s0 = None if s0shape is None else leaf("shifted0", s0shape)
        out = route(label + " forward", mix_op.ddlerp, x, maa, m, s0, **kw)
        route(label + " backward", out.backward, t("dout", tuple(out.shape), bf))

    ddlerp("ddlerp dense", (B, T, C), (B, C), True)
    ddlerp("ddlerp dense no m no shifted0", (B, T, C), None, False)
    ddlerp("ddlerp dense rev", (B, T, C), (B, C), True, rev_n=rev_b)
    ddlerp("ddlerp varlen", (1, TOTAL, C), (NSEQ, C), True, cu_seqlens=cu)
    ddlerp("ddlerp varlen no m no shifted0", (TOTAL, C), None, False, cu_seqlens=cu)
    ddlerp("ddlerp varlen rev", (1, TOTAL, C), (NSEQ, C), True, cu_seqlens=cu, rev_n=rev_s)
    ddlerp("ddlerp varlen rev no m no shifted0", (TOTAL, C), None, False, cu_seqlens=cu, rev_n=rev_s)

    # ---- mix_op: the slot-pool ops and LoRA (inference only)
    with torch.no_grad():
        x, spool = t("x", (1, TOTAL, C), bf), t("shift_pool", (4, C), bf)
        slots = ints("slots", (1, 0))
        route("ddlerp_slots NS 5 m slots", mix_op.ddlerp_slots, x, t("maa", (5, C), bf), t("m", (5, 1, TOTAL, C), bf), spool, slots, cu)
        route("ddlerp_slots NS 1", mix_op.ddlerp_slots, x, t("maa", (1, 1, C), bf), None, spool, None, cu)
        route("ddlerp_slots NS 2", mix_op.ddlerp_slots, t("x", (TOTAL, C), bf), t("maa", (2, C), bf), None, spool, slots, cu)
        route("shift_keep", mix_op.shift_keep, x, cu, 5, spool, None)
        route("shift_keep slot_out", mix_op.shift_keep, x, cu, 1 << 40, spool, ints("slot_out", (3, 2)))
        route("shift_keep snap", mix_op.shift_keep, x, cu, 5, spool, ints("slot_out", (3, 2)),
              (64, ints("cu_snap", (0, 0, 1)), ints("snap_slots", (2,))))
        route("shift_keep snap_every 0", mix_op.shift_keep, x, cu, 5, spool, None, (0, ints("cu_snap", (0, 0, 0)), None))
        K, R = 64, 8
        route("lora_packed", mix_op.lora_packed, t("x", (1, TOTAL, K), bf), t("y", (1, TOTAL, K), bf), t("A_pool", (2, R, K), bf),
              t("B_pool", (2, K, R), bf), t("scale", (2,), f32), ints("adapter", (1, -1)), cu)

    # ---- mix_op: GroupNorm * gate and the FFN glue, forward and backward through autograd
    y, g, gamma, beta = leaf("y", (B * T, C)), leaf("g", (B * T, C)), leaf("gamma", (C,)), leaf("beta", (C,))
    out = route("group_norm_gate forward", mix_op.group_norm_gate, y, g, gamma, beta, H, 64e-5)
    route("group_norm_gate backward", out.backward, t("dout", (B * T, C), bf))
    x = leaf("x", (B, T, C))
    out = route("sqrelu forward", mix_op.sqrelu, x)
    route("sqrelu backward", out.backward, t("dout", (B, T, C), bf))
    r, kv = leaf("r", (B, T, C)), leaf("kv", (B, T, C))
    out = route("sigmoid_mul forward", mix_op.sigmoid_mul, r, kv)
    route("sigmoid_mul backward", out.backward, t("dout", (B, T, C), bf))
    torch.cuda.synchronize()
    return rec.records


def recorded(patch):
    """patch(obj, name, value): how `_lib.load` and `_lib._selftested` are replaced (monkeypatch.setattr, or plain setattr)."""
    import torch
    from rwkv_lm_ext_amd import _lib
    rec = Recorder(torch)
    patch(_lib, "load", lambda: rec)
    patch(_lib, "_selftested", set(range(torch.cuda.device_count())))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        records = record(torch, rec)
    torch.cuda.current_stream().wait_stream(side)
    return json.loads(json.dumps(records))


def test_every_wrapper_makes_the_recorded_library_calls(monkeypatch):
    got = recorded(monkeypatch.setattr)
    with open(EXPECTED) as fh:
        want = json.load(fh)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"record {i}, wrapper {g[0]!r}: the library call differs from the recorded one\n got  {g}\n want {w}"
    assert len(got) == len(want), f"{len(got)} library calls, {len(want)} recorded; first surplus: {(got + want)[min(len(got), len(want))]}"
    assert len({g[0] for g in got}) > 100 and all(any(s == "stream" for s in g[2]) for g in got if not g[1].endswith("_bytes"))


def test_refusals_that_need_a_gpu_tensor_launch_nothing(monkeypatch):
    """Each row: (call, exception type, full message, whether the library is loaded before the refusal).  The last column is the parent's
    order: a refusal that came before `_lib.load()` must not move behind it."""
    import torch
    from rwkv_lm_ext_amd import _lib, mix_op, wkv6_op as op
    rec, loads = Recorder(torch), []

    def load():
        loads.append(1)
        return rec

    monkeypatch.setattr(_lib, "load", load)
    monkeypatch.setattr(_lib, "_selftested", set(range(torch.cuda.device_count())))
    early, late = False, True
    bf, f32, i32 = torch.bfloat16, torch.float32, torch.int32
    z = lambda *shape, dtype=bf: torch.zeros(shape, dtype=dtype, device="cuda")
    r, u, cu = z(B, T, C), z(H, N), torch.tensor(CU, dtype=i32, device="cuda")
    p = z(TOTAL, C)
    rows = [
        # _check_tensors, in its order per tensor: dtype after is_cuda, contiguity, shape; then C == H*64
        (early, lambda: op.forward_ex(r, r.float(), r, r, u, H), RuntimeError, "k must be torch.bfloat16, got torch.float32"),
        (early, lambda: op.forward_ex(r, r, z(B, T, 2 * C)[:, :, ::2], r, u, H), RuntimeError, "v must be contiguous"),
        (early, lambda: op.forward_ex(r, r, r, z(B, T + 1, C), u, H), RuntimeError,
         f"w has shape {(B, T + 1, C)}, expected {(B, T, C)}"),
        (early, lambda: op.forward_ex(r, r.cpu(), r, r, u, H), RuntimeError, "k must be on the GPU (the WKV6 operator has no CPU path)"),
        (early, lambda: op.forward_ex(r, r, r, r, z(1, N), 1), RuntimeError, f"C ({C}) must equal H*64 (64)"),
        (early, lambda: op.wkv6_cuda.forward(B, T, C, H, r, r, r, r, u, r), RuntimeError, "w must be torch.float32, got torch.bfloat16"),
        (early, lambda: op.wkv6state_cuda.forward(B, T, C, H, r, r, r, r, u, z(B, H, N, N), r), RuntimeError,
         f"s has shape {(B, H, N, N)}, expected {(H, N, N)}"),
        (early, lambda: op.rwkv6.forward_bf16(B, T, C, H, z(B, H, N, 32, dtype=f32), r, r, r, r.float(), u, r), RuntimeError,
         f"state has shape {(B, H, N, 32)}, expected (-1,)"),
        # an int array that is not on the device of the tensors
        (late, lambda: op.forward_rev_ex(r, r, r, r, u, H, torch.zeros(B, dtype=i32), 0), RuntimeError,
         "rev_n must be a contiguous int32 [B] tensor on the device of r"),
        (late, lambda: op.forward_rev_ex(r, r, r, r, u, H, z(B, dtype=i32), 32), RuntimeError, "rev_mask 32 has unknown bits"),
        (early, lambda: op.forward_varlen_ex(p, p, p, p, u, H, cu.cpu(), 5), RuntimeError,
         "cu_seqlens must be a contiguous int32 [n_seq + 1] tensor on the device of r"),
        (late, lambda: op.forward_varlen_rev_ex(p, p, p, p, u, H, cu, 5, torch.zeros(NSEQ, dtype=i32), 0), RuntimeError,
         "rev_n must be a contiguous int32 [n_seq] tensor on the device of r"),
        (early, lambda: op.rwkv6.forward_varlen_bf16(TOTAL, C, H, z(4, H, N, N, dtype=f32), torch.zeros(NSEQ, dtype=i32), p, p, p, p.float(), u, p, cu,
                                              8), RuntimeError,
         "state_slot must be a contiguous int32 [n_seq] tensor on the device of r, or None"),
        (early, lambda: op.rwkv6.forward_varlen_bf16(TOTAL, C, H, z(4, H, N, N, dtype=f32), None, p, p, p, p.float(), u, p, cu, 8,
                                              ws=torch.zeros(64, dtype=torch.uint8)), RuntimeError,
         "ws must be a new_rwkv6_varlen_workspace() buffer on the device of r"),
        (late, lambda: op.forward_pair_ex(H, u, [dict(r=r, k=r, v=r, w=r, rev_n=z(B + 1, dtype=i32))] * 2), RuntimeError,
         "rev_n must be a contiguous int32 [B] tensor on the device of r"),
        (late, lambda: op.backward_pair_ex(H, u, [dict(r=r, k=r, v=r, w=r, gy=r)] * 2), RuntimeError,
         "wkv6 pair backward: both problems need the checkpoints their forward wrote"),
        (late, lambda: op.backward_varlen_pair_ex(H, u, [dict(r=p, k=p, v=p, w=p, gy=p)] * 2, cu, 5), RuntimeError,
         "wkv6 packed pair backward: both problems need the workspaces their forward wrote"),
        (early, lambda: op.bi_forward_ex(z(B, T, dtype=i32).long(), r, r, r, r, u, H), RuntimeError, "mask must be torch.int32, got torch.int64"),
        (late, lambda: op.backward_varlen_ex(p, p, p, p, u, p, H, cu, 5, ckpt_valid=True), RuntimeError,
         "ckpt_valid needs the workspace the forward filled"),
        (late, lambda: op.backward_varlen_rev_ex(p, p, p, p, u, p, H, cu, 5, None, 0, ckpt_valid=True), RuntimeError,
         "ckpt_valid needs the workspace the forward filled"),
        (early, lambda: torch.ops.wkv6.forward_varlen(TOTAL + 1, C, H, p, p, p, p, u, cu, 5, p), RuntimeError,
         f"r has shape {(TOTAL, C)}, expected {(TOTAL + 1, C)}"),
        (early, lambda: mix_op.sigmoid_mul(r, p), RuntimeError, "sigmoid_mul: r and kv must have the same shape"),
        # mix_op: the device is judged last
        (early, lambda: mix_op.ddlerp(r, z(5, C), rev_n=torch.zeros(B, dtype=i32)), RuntimeError,
         "rev_n must be a contiguous int32 [B] tensor on the device of x"),
        (early, lambda: mix_op.ddlerp(p, z(5, C), cu_seqlens=cu.cpu()), RuntimeError,
         "cu_seqlens must be a contiguous int32 [n_seq + 1] tensor on the device of x"),
        (early, lambda: mix_op.ddlerp(p, z(5, C), cu_seqlens=cu, rev_n=z(NSEQ + 1, dtype=i32)), RuntimeError,
         "rev_n must be a contiguous int32 [n_seq] tensor on the device of x"),
        (early, lambda: mix_op.ddlerp(z(2, TOTAL, C), z(5, C), cu_seqlens=cu), RuntimeError, "a packed batch is [1, total_T, C] (or [total_T, C])"),
        (early, lambda: mix_op.ddlerp(p, z(5, C), shifted0=z(3, C), cu_seqlens=cu), RuntimeError, f"shifted0 must be [n_seq, C] = {(NSEQ, C)}"),
        (early, lambda: mix_op.ddlerp_slots(p, z(1, C), None, z(4, C), None, cu.cpu()), RuntimeError,
         "shift_pool and cu_seqlens must be on the device of x"),
        (early, lambda: mix_op.ddlerp_slots(p, z(1, C), None, z(4, C), torch.zeros(NSEQ, dtype=i32), cu), RuntimeError,
         "maa, m and slots must be on the device of x"),
        (early, lambda: mix_op.shift_keep(p, cu, 5, z(4, C), torch.zeros(NSEQ, dtype=i32)), RuntimeError,
         "slot_out must be a contiguous int32 tensor on the device of x"),
        (early, lambda: mix_op.lora_packed(z(TOTAL, 64), z(TOTAL, 64), z(2, 8, 64), z(2, 64, 8), z(2, dtype=f32), torch.zeros(NSEQ, dtype=i32), cu),
         RuntimeError, "y, A_pool, B_pool, scale, adapter and cu_seqlens must be on the device of x"),
    ]
    with torch.no_grad():
        for i, (loaded, call, exc, message) in enumerate(rows):
            del loads[:]
            with pytest.raises(exc) as info:
                call()
            assert type(info.value) is exc and str(info.value) == message, f"row {i}: {type(info.value).__name__}: {info.value}"
            assert bool(loads) == loaded, f"row {i} ({message}): the library was {'loaded' if loads else 'not loaded'} before the refusal"
    assert [rec_ for rec_ in rec.records if not rec_[1].endswith("_bytes")] == []


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    print("[\n" + ",\n".join(json.dumps(rec) for rec in recorded(setattr)) + "\n]")
