#!/usr/bin/env python3
"""The organizers' Subtask-2B training step (example_scripts/ResNet_example_task2B.py: ``ResNetConfig(num_channels=1, layer_type="basic",
depths=[2, 2], hidden_sizes=[32, 64])``, batch 16, 224 x 224 grayscale): steps per second of ``HFResNetForImageClassification`` on the
HIP tower, and of transformers' ``ResNetForImageClassification`` under torch on the same GPU.

A step = forward + cross entropy + backward + one Adam step.  Settings, alternated on the same GPU:

  hip_resident    memehip model (fp16 storage, fused Adam over flat buffers), the batch a device-resident f32 tensor
  hip_pipeline    the same, every step's batch made by ``DeviceImagePipeline(grayscale=True)`` from 16 decoded uint8 arrays (400 x 300)
  torch_fp32      transformers' module, torch.optim.AdamW, device-resident batch
  torch_amp_fp16  the same under torch.autocast(float16) with a GradScaler

Per setting and alternation: --warmup steps, then --windows windows of --steps steps, ONE device synchronise per window; a setting's figure
is the median over its windows and alternations.  One more instrumented pass of the HIP model puts device events around every
convolution's input-gradient launch (``_Conv.backward``: the weight gradients are queued, not launched, inside it) and reports the share
of the step that the layers on the panel routes (GEMM / GEMM + col2im: Cout % 64 != 0) take -- the basis for a later decision about a
narrower tile.  --profile N: only N untimed steps of hip_resident (the run to put under ``rocprofv3 --kernel-trace --stats``).

  python tools/task2b_bench.py --out profiles/r22_task2b.json

Context only: the reference's own 2B run is 8.12 samples/s on another machine, bound by image decoding on the host.
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

EXAMPLE = dict(num_channels=1, layer_type="basic", depths=[2, 2], hidden_sizes=[32, 64], num_labels=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--image-size", type=int, default=224)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed window (one synchronise per window)")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--step-limit", type=float, default=2.0, help="abort when a window averages more than this many seconds per step")
    ap.add_argument("--profile", type=int, default=0, help="N > 0: run N steps of hip_resident and exit (for a profiler)")
    ap.add_argument("--no-torch", action="store_true", help="leave the transformers / torch settings out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("task2b_bench: needs the GPU (a CPU run measures nothing)")
    import multimodal_propaganda_meme_classification_amd as pkg
    R = pkg.resnet
    B, S = args.batch, args.image_size
    g = torch.Generator().manual_seed(1)
    resident = torch.randn((B, 1, S, S), generator=g).cuda()
    labels = torch.randint(0, 2, (B,), generator=g).cuda()
    rng = np.random.default_rng(2)
    decoded = [rng.integers(0, 256, (300, 400, 3), dtype=np.uint8) for _ in range(B)]
    pipe = pkg.data.DeviceImagePipeline(S, 256, "center_crop", device="cuda", grayscale=True, mean=(0.45,), std=(0.22,))

    model = pkg.HFResNetForImageClassification(**EXAMPLE, compute_dtype="fp16", seed=0).cuda().train()
    pkg.flatten_parameters(model)
    opt = pkg.Adam(model.parameters(), lr=2e-5)

    def hip_step(x):
        opt.zero_grad()
        loss, _ = model(pixel_values=x, labels=labels)
        loss.backward()
        opt.step()

    settings = {"hip_resident": lambda: hip_step(resident), "hip_pipeline": lambda: hip_step(pipe(decoded))}
    if args.profile:
        for _ in range(args.profile):
            settings["hip_resident"]()
        torch.cuda.synchronize()
        return
    if not args.no_torch:
        from transformers import ResNetConfig, ResNetForImageClassification
        torch.manual_seed(0)
        hf = ResNetForImageClassification(ResNetConfig(**EXAMPLE)).cuda().train()
        hf_opt = torch.optim.AdamW(hf.parameters(), lr=2e-5)
        scaler = torch.amp.GradScaler("cuda")

        def torch_step(amp):
            hf_opt.zero_grad()
            if amp:
                with torch.autocast("cuda", dtype=torch.float16):
                    loss = hf(pixel_values=resident, labels=labels).loss
                scaler.scale(loss).backward()
                scaler.step(hf_opt)
                scaler.update()
            else:
                hf(pixel_values=resident, labels=labels).loss.backward()
                hf_opt.step()
        settings["torch_fp32"] = lambda: torch_step(False)
        settings["torch_amp_fp16"] = lambda: torch_step(True)

    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    medians = {name: [] for name in settings}
    for alt in range(args.alternations):
        for name, step in settings.items():
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
                    raise SystemExit(f"task2b_bench: {dt:.2f} s per step exceeds --step-limit {args.step_limit}")
                per_step.append(dt)
            med = statistics.median(per_step)
            medians[name].append(med)
            emit({"what": "step_time", "setting": name, "alternation": alt, "median_ms": round(med * 1e3, 4), "min_ms": round(min(per_step) * 1e3, 4),
                  "max_ms": round(max(per_step) * 1e3, 4), "steps": args.steps * args.windows})

    # ---- the panel routes' share of the HIP step: device events around every convolution's input-gradient launch ----
    tower = model.resnet
    names = {id(u.conv): n for n, m in model.named_modules() for u in tower._units if u.conv.mod is m}
    spans, real = [], R._Conv.backward

    def timed(self, lib, dy, x, wk, Bn, H, W, *a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = real(self, lib, dy, x, wk, Bn, H, W, *a, **kw)
        e1.record()
        need_dx = kw.get("need_dx", a[5] if len(a) > 5 else True)          # (a: Ho, Wo, gscale, wjobs, opts, need_dx)
        spans.append((names[id(self)], R.dgrad_route(self, H, W, tower.options) if need_dx else "none", e0, e1))
        return out
    n_inst = 20
    R._Conv.backward = timed
    try:
        s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        hip_step(resident)
        torch.cuda.synchronize()
        del spans[:]
        s0.record()
        for _ in range(n_inst):
            hip_step(resident)
        s1.record()
        torch.cuda.synchronize()
    finally:
        R._Conv.backward = real
    total_ms = s0.elapsed_time(s1) / n_inst
    per_layer = {}
    for name, route, e0, e1 in spans:
        ms, _ = per_layer.get(name, (0.0, route))
        per_layer[name] = (ms + e0.elapsed_time(e1) / n_inst, route)
    panel_ms = sum(ms for ms, route in per_layer.values() if route in (R.GEMM, R.COL2IM))
    implicit_ms = sum(ms for ms, route in per_layer.values() if route == R.IMPLICIT)
    emit({"what": "input_gradient_routes", "instrumented_step_ms": round(total_ms, 4), "panel_routes_ms": round(panel_ms, 4),
          "implicit_routes_ms": round(implicit_ms, 4), "panel_share_of_step": round(panel_ms / total_ms, 4),
          "layers": {n: {"route": r, "ms": round(ms, 4)} for n, (ms, r) in per_layer.items()},
          "note": "event spans include launch gaps; the weight gradients are launched outside these spans"})

    fig = {name: statistics.median(v) for name, v in medians.items()}
    spread = max(max(v) - min(v) for v in medians.values())
    rec = {"what": "summary", "model": "ResNetConfig" + json.dumps(EXAMPLE), "batch": B, "image_size": S, "step": "forward + loss + backward + Adam",
           "run_to_run_spread_ms": round(spread * 1e3, 4), "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "reference_context_samples_per_s": 8.12, "reference_context_note": "BASELINE.md 2B row: another machine, host decode bound"}
    for name, t in fig.items():
        rec[f"{name}_ms"] = round(t * 1e3, 4)
        rec[f"{name}_steps_per_s"] = round(1.0 / t, 2)
        rec[f"{name}_samples_per_s"] = round(B / t, 1)
    emit(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
