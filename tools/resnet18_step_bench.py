#!/usr/bin/env python3
"""ResNet-18 image tower (the submitted Subtask-2C model's, example_scripts/Multimodal_example_task2C.py:569-574), forward + backward:
step time with ``TowerOptions.pair_dgrad`` on and off, alternated on the same GPU, and the launches per step.

Batch 32, 224 x 224, fp16, ``features(image)`` + a fixed upstream gradient (no head, no optimizer: the tower alone).  Per setting and
alternation: --warmup steps, then --windows windows of --steps steps each, ONE device synchronise per window; the step time of a
window is its wall time / steps, a setting's figure the median over its windows (>= 50 steps in all).  A window that takes longer
than --step-limit seconds per step aborts the run.  Launches per step: the libmemehip entry points the tower calls, counted by
wrapping the library handle for one step (every entry point is one launch, except the split-K forward / dgrad convolutions' two).
One JSON line per setting and alternation, then a summary line; --out also writes them to a file.

  python tools/resnet18_step_bench.py --out profiles/r06_resnet18_pair_dgrad.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def count_launches(pkg, net, step):
    """libmemehip calls of one step (name -> count), by wrapping every mh_* entry point of the handle the tower uses"""
    lib = pkg._lib.load(net.compute_dtype)
    skip = ("mh_conv_splitk", "mh_bn2d_workspace_elems", "mh_gemm_ksplit_for", "mh_status_str", "mh_version")      # host-only queries
    names = [n for n in pkg._lib.EXPORTED_SYMBOLS if n not in skip]
    counts, real = {}, {}
    for n in names:
        real[n] = getattr(lib, n)

        def wrapped(*a, _n=n):
            counts[_n] = counts.get(_n, 0) + 1
            return real[_n](*a)
        setattr(lib, n, wrapped)
    try:
        step()
        torch.cuda.synchronize()
    finally:
        for n, f in real.items():
            setattr(lib, n, f)
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--image-size", type=int, default=224)
    ap.add_argument("--dtype", choices=("fp16", "bf16"), default="fp16")
    ap.add_argument("--layers", type=int, nargs=4, default=(2, 2, 2, 2))
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed window (one synchronise per window)")
    ap.add_argument("--windows", type=int, default=6, help="timed windows per setting and alternation (steps x windows >= 50)")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--step-limit", type=float, default=2.0, help="abort when a window averages more than this many seconds per step")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resnet18_step_bench: needs the GPU (a CPU run measures nothing)")
    if args.steps * args.windows < 50:
        raise SystemExit("resnet18_step_bench: steps x windows must be >= 50")
    import multimodal_propaganda_meme_classification_amd as pkg

    net = pkg.ResNet18(num_classes=0, compute_dtype=args.dtype, layers=tuple(args.layers), seed=0).cuda().train()
    pkg.flatten_parameters(net)          # f32 .grad views: the gradients are accumulated in place, as under the fused Adam
    g = torch.Generator().manual_seed(1)
    image = torch.randn((args.batch, 3, args.image_size, args.image_size), generator=g).cuda()
    upstream = (torch.randn((args.batch, net.feature_dim), generator=g) * 1e-3).cuda()

    def step():
        (net.features(image) * upstream).sum().backward()

    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    settings = {"pair_dgrad=1": pkg.TowerOptions(pair_dgrad=True), "pair_dgrad=0": pkg.TowerOptions(pair_dgrad=False)}
    launches = {}
    for name, opts in settings.items():
        net.options = opts
        step()
        torch.cuda.synchronize()
        c = count_launches(pkg, net, step)
        launches[name] = sum(c.values())
        emit({"what": "launches_per_step", "setting": name, "library_calls": launches[name], "mh_conv_dgrad_pair": c.get("mh_conv_dgrad_pair", 0),
              "mh_col2im_nhwc": c.get("mh_col2im_nhwc", 0), "mh_gemm_bf16_grouped": c.get("mh_gemm_bf16_grouped", 0), "mh_add_h16": c.get("mh_add_h16", 0),
              "mh_conv_dgrad": c.get("mh_conv_dgrad", 0)})
    medians = {name: [] for name in settings}
    for alt in range(args.alternations):
        for name, opts in settings.items():
            net.options = opts
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            per_step = []
            for _ in range(args.windows):
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / args.steps
                if dt > args.step_limit:
                    raise SystemExit(f"resnet18_step_bench: {dt:.2f} s per step exceeds --step-limit {args.step_limit}")
                per_step.append(dt)
            med = statistics.median(per_step)
            medians[name].append(med)
            emit({"what": "step_time", "setting": name, "alternation": alt, "median_ms": round(med * 1e3, 4), "min_ms": round(min(per_step) * 1e3, 4),
                  "max_ms": round(max(per_step) * 1e3, 4), "steps": args.steps * args.windows})
    on, off = medians["pair_dgrad=1"], medians["pair_dgrad=0"]
    spread = max(max(v) - min(v) for v in medians.values())
    m_on, m_off = statistics.median(on), statistics.median(off)
    emit({"what": "summary", "tower": f"ResNet18{tuple(args.layers)}", "batch": args.batch, "image_size": args.image_size, "dtype": args.dtype,
          "forward_backward_only": True, "pair_dgrad=1_ms": round(m_on * 1e3, 4), "pair_dgrad=0_ms": round(m_off * 1e3, 4),
          "run_to_run_spread_ms": round(spread * 1e3, 4), "pair_slower_than_spread": bool(m_on - m_off > spread),
          "images_per_s_pair_dgrad=1": round(args.batch / m_on, 1), "images_per_s_pair_dgrad=0": round(args.batch / m_off, 1),
          "launches_per_step": launches, "device": torch.cuda.get_device_name(0)})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
