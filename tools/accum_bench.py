#!/usr/bin/env python
"""What gradient accumulation costs per micro-batch (config 3: ViT-B/16 + BERT-base, 224 x 224, S = 128, batch 32, eager
autograd path: forward, loss, backward).

Three ways to run a micro-batch that is not the first of its window, timed in the same process, alternating:

  (a) overwrite   the switch off: the backward overwrites .grad (what the parent commit does; no accumulation at all)
  (b) add         set_grad_accumulation(True): the weight gradients are added in the GEMM epilogue, the word-table rows in place,
                  the small gradients through the scratch mirror and one mh_accum_spans_f32 launch
  (c) naive       the overwriting backward, then one full-buffer ``acc.add_(model.flat_grads)``

(b) must not be slower than (c): otherwise accumulating inside the epilogue has not paid for its code.  Every variant is warmed
up, then the three are run round-robin for ``--rounds`` rounds of ``--iters`` micro-batches each, every round timed by a host clock
around work that ends in a device synchronise; the medians over the rounds are reported and written to ``--out``.

    python tools/accum_bench.py [--tiny] [--rounds 7] [--iters 20] [--out profiles/r19_grad_accum.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_propaganda_meme_classification_amd as pkg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiny", action="store_true", help="tiny model (rehearsal only; not a measurement)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="fp16")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("accum_bench: needs the GPU (no CPU timing stands in for it)")
    if args.tiny:
        cfg = pkg.ModelConfig(text=pkg.TextConfig(vocab_size=512, hidden=128, layers=2, heads=2, intermediate=256, max_position=64),
                              image=pkg.ImageConfig(image_size=32, hidden=128, layers=2, heads=2, intermediate=256), proj=128)
        B, S = 4, 16
    else:
        cfg, B, S = pkg.ModelConfig(), args.batch, args.seq
    cfg.compute_dtype = args.dtype
    model = pkg.MultimodalClassifier.from_config(cfg, seed=0).to("cuda").train()
    crit = pkg.CrossEntropyLoss()
    g = torch.Generator().manual_seed(1)
    text = torch.randint(5, cfg.text.vocab_size, (B, S), generator=g)
    lens = torch.randint(max(2, S // 4), S + 1, (B,), generator=g)
    mask = (torch.arange(S)[None] < lens[:, None]).long()
    text = (text * mask).cuda()
    mask = mask.cuda()
    image = torch.randn((B, 3, cfg.image.image_size, cfg.image.image_size), generator=g).cuda()
    labels = torch.randint(0, 2, (B,), generator=g).cuda()
    acc = torch.zeros_like(model.flat_grads)

    def micro_batch():
        crit(model(text, image, mask), labels).backward()

    def overwrite():
        model.set_grad_accumulation(False)
        micro_batch()

    def add():
        micro_batch()          # the switch is on and nothing cleared the gradients: the adding backward

    def naive():
        model.set_grad_accumulation(False)
        micro_batch()
        acc.add_(model.flat_grads)

    def prepare_add():
        model.set_grad_accumulation(True)
        micro_batch()          # opens a window (overwrites); every later one adds
        torch.cuda.synchronize()

    def close_window():
        overwrite()            # untimed: the next overwriting backward clears the word-table rows the window's adds touched
        torch.cuda.synchronize()

    variants = (("overwrite", overwrite, None, None), ("add", add, prepare_add, close_window), ("naive", naive, None, None))
    for _, fn, prep, post in variants:
        if prep:
            prep()
        for _ in range(args.warmup):
            fn()
        if post:
            post()
        torch.cuda.synchronize()
        model.flat_grads.zero_()
    times = {name: [] for name, *_ in variants}
    for _ in range(args.rounds):
        for name, fn, prep, post in variants:
            if prep:
                prep()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.iters * 1e3)
            if post:
                post()
            model.flat_grads.zero_()       # (keeps the sums of the adding variant finite over the rounds)
    ms = {name: statistics.median(v) for name, v in times.items()}
    n_total, n_shadow = model.layout.n_total, model.layout.n_shadow
    out = {
        "what": "time per micro-batch (forward + loss + backward, eager autograd path), milliseconds: median over the rounds",
        "config": "tiny (rehearsal)" if args.tiny else "config 3", "batch": B, "seq": S, "dtype": args.dtype,
        "rounds": args.rounds, "iters_per_round": args.iters,
        "overwrite_ms": ms["overwrite"], "add_ms": ms["add"], "naive_add_ms": ms["naive"],
        "spread_ms": {name: [min(v), max(v)] for name, v in times.items()},
        "add_not_slower_than_naive": ms["add"] <= ms["naive"],
        "flat_buffer_bytes": 4 * n_total, "matrix_gradient_bytes": 4 * n_shadow,
        "device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
        "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "torch": torch.__version__, "hip": torch.version.hip,
    }
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
