"""Time the LoRA bi-encoder training step of bench.py --workload dp_lora (BASELINE configs[3]: 24 layers, C = 2048, dim_ffn = 7168, per-GPU
batch 32 triples = 96 rows of T = 512, activation checkpointing, DDP over a one-rank RCCL group, AdamW on the LoRA / dense parameters) fed

  padded       the three [32, 512] batches of train_dp.batches, as the benchmark feeds them
  packed/1     the same rows as one packed batch (train_dp.batches(packed=True)): every row cut behind its emb_id token
  packed/256   ... with total_T rounded up to a multiple of 256 (rows that belong to no sequence), which bounds the GEMM shapes a run sees

on (a) the benchmark's own synthetic batches (n uniform in 16..510, n + 1 tokens kept of 512) and (b) a batch of full-length rows (emb_id
at position 511: nothing to leave out, packing can only cost).

Method: the alternated rounds of tools/timing.py around the benchmark's own timing.  One process, one model, one optimizer; the batches
of a case are made once, staged in pinned memory, and every contender walks the same list.  A contender's time is dp.timed_steps (the benchmark's timing: --warmup untimed steps, then --steps steps between device
synchronisations) and the contenders alternate within each of --rounds rounds; reported is ms per step, median [min, max] over the rounds,
every round listed.  The batches differ in their token counts, so with total_multiple = 1 nearly every step of a round is a GEMM shape the
process has not run before in round 1 and a repeated one afterwards: round 1 is what a real epoch sees.  The optimizer keeps stepping
through all of it, so the "last loss" of two contenders is of the same batch under slightly different weights: a sanity figure only.

    python tools/time_train_packed.py [--layers 24] [--steps 5] [--warmup 2] [--rounds 3] [--out profiles/train_packed_time.txt]
"""
import argparse
import os
import socket
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VOCAB, N_EMBD, DIM_FFN, T = 65536, 2048, 7168, 512


def build(layers, dev):
    """the model of bench.bench_dp_lora, wrapped and with its optimizer"""
    import torch
    import torch.distributed as dist
    from rwkv_lm_ext_amd import train_dp
    torch.manual_seed(0)
    with torch.device(dev):
        model = train_dp.SequenceEmbedder(VOCAB, N_EMBD, layers, dim_ffn=DIM_FFN, add_mlp=True, output_dim=1024, grad_cp=True).to(torch.bfloat16)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.dim() >= 2 and "emb" not in n:
                p.normal_(0.0, 0.02)
            if "time_decay" in n and p.dim() == 3:
                p.copy_(torch.linspace(-6, -1, p.numel(), device=dev).view_as(p))
            if "ln_x.weight" in n or (n.endswith(".weight") and ".ln" in n):
                p.fill_(1.0)
    train_dp.inject_lora(model, r=8, alpha=32)
    for p in model.dense.parameters():
        p.requires_grad_(True)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("lora_B"):
                p.normal_(0.0, 0.01)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if "MASTER_PORT" not in os.environ:
        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0))
            os.environ["MASTER_PORT"] = str(sock.getsockname()[1])
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    net = train_dp.wrap_ddp(model, dev)
    opt = torch.optim.AdamW(train_dp.trainable_parameters(model), lr=1e-5)
    model.train()
    return model, net, opt, dist


def full_rows(index, bs):
    """3 * bs rows of T - 1 ordinary tokens and the emb_id token at position T - 1"""
    import torch
    g = torch.Generator().manual_seed(7000003 * index + 5)
    rows = torch.randint(2, VOCAB, (3 * bs, T), generator=g)
    rows[:, T - 1] = 1
    return rows


def make_batches(case, count, bs):
    """{contender: [batch, ...]} over the same rows, in pinned memory"""
    import torch
    from rwkv_lm_ext_amd import train_dp
    from rwkv_lm_ext_amd.dp import BucketBatchSampler
    if case == "synthetic":
        dense = list(train_dp.batches(BucketBatchSampler([count * bs], [bs], 0, 1), T, VOCAB))
    else:
        dense = []
        for i in range(count):
            rows = full_rows(i, bs)
            dense.append({"query": rows[:bs], "positive": rows[bs:2 * bs], "negative": rows[2 * bs:]})
    out = {"padded": dense}
    for mult in (1, 256):
        packed = []
        for b in dense:
            idx, cu, max_seqlen, actual = train_dp.pack_rows(torch.cat([b["query"], b["positive"], b["negative"]]), total_multiple=mult)
            packed.append({"idx": idx, "cu_seqlens": cu, "max_seqlen": max_seqlen, "actual_len": actual, "bs": bs})
        out[f"packed/{mult}"] = packed
    pin = lambda b: {k: v.pin_memory() if isinstance(v, torch.Tensor) else v for k, v in b.items()}
    return {name: [pin(b) for b in bs_] for name, bs_ in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--per-gpu-batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from rwkv_lm_ext_amd import train_dp
    from rwkv_lm_ext_amd.dp import timed_steps
    if not torch.cuda.is_available():
        sys.exit("time_train_packed.py needs the GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    model, net, opt, dist = build(args.layers, dev)
    log = timing.Log()
    say = log.say

    say(f"time_train_packed.py: {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {args.layers} layers, C = {N_EMBD}, dim_ffn = "
        f"{DIM_FFN}, {3 * args.per_gpu_batch} rows of T = {T} a step, grad checkpointing, DDP world size 1; {args.rounds} rounds of "
        f"{args.warmup} warm-up + {args.steps} timed steps per contender (dp.timed_steps), contenders alternating; ms per step")
    count = args.steps + args.warmup
    for case in ("synthetic", "full-length"):
        batches = make_batches(case, count, args.per_gpu_batch)
        real = sum(int(b["cu_seqlens"][-1]) for b in batches["packed/1"]) / count
        rows256 = sum(b["idx"].shape[1] for b in batches["packed/256"]) / count
        say()
        say(f"case {case}: {real:.0f} of {3 * args.per_gpu_batch * T} tokens a step are in front of or at the emb_id token "
            f"({100 * real / (3 * args.per_gpu_batch * T):.1f} %); packed/256 runs {rows256:.0f} rows a step")
        last = {}

        def contender(name):
            it = iter(batches[name])

            def step():
                batch = train_dp.to_device(next(it), dev)
                opt.zero_grad(set_to_none=True)
                if "idx" in batch:
                    loss = train_dp.training_loss(net, batch)
                else:
                    loss = train_dp.training_loss(net, batch["query"], batch["positive"], batch["negative"])
                loss.backward()
                opt.step()
                last[name] = loss.detach()
            return step

        for name in batches:                                    # allocator / module-load warm-up, outside the warm-up steps (bench.py)
            one = contender(name)
            one()
        torch.cuda.synchronize()
        ms_per_step = lambda name: timed_steps(contender(name), args.steps, args.warmup, torch.cuda.synchronize, dist, dev) * 1e3 / args.steps
        times = timing.alternate({name: name for name in batches}, ms_per_step, args.rounds)
        base = timing.median(times["padded"])
        for name, ts in times.items():
            med = timing.median(ts)
            say(f"  {name:<11} {med:8.2f} [{min(ts):8.2f}, {max(ts):8.2f}]   x{med / base:5.3f} of padded   rounds: "
                + ", ".join(f"{t:.2f}" for t in ts) + f"   last loss {float(last[name]):.4f}")
    dist.destroy_process_group()
    log.write(args.out)


if __name__ == "__main__":
    main()
