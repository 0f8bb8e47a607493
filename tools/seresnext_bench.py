#!/usr/bin/env python3
"""SE-ResNeXt-50 32x4d on the MI355X: the five squeeze-and-excitation kernels at the real layer shapes, and the whole training step
against ResNeXt-50 32x4d.

1. Per kernel: mh_se_gate_fwd / mh_se_apply_fwd / mh_se_apply_bwd_reduce / mh_se_gate_bwd / mh_se_apply_bwd at the four SE shapes of the tower
   at batch 32, 224 x 224 input (C = 256 @ 56^2, 512 @ 28^2, 1024 @ 14^2, 2048 @ 7^2; R = 16 / 32 / 64 / 128).  HIP events around --iters
   launches, --reps windows, the median and the spread.  "bytes" is what the kernel must move (every operand read once, every output
   written once), "TBps" that over the median time.  Back-to-back launches over the same tensors: operands up to the Infinity Cache's size
   stay cache-resident between launches, so the small layers' rates are cache rates, not HBM rates (the step's are lower).
2. Whole step: ResNetClassifier, batch 32, 224^2, fp16, forward + cross entropy + backward + Adam -- seresnext50_32x4d against
   resnext50_32x4d, alternated on one device in one session.  Reported, not gated.  --kernel-stats FILE: a ``rocprofv3 --kernel-trace --stats``
   CSV of a ``--profile N`` run (a run of its own); the SE kernels' share of the kernel time goes into the summary.

  python tools/seresnext_bench.py --out profiles/r30_seresnext.json
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

# (layer, C, H = W at 224 px, R)
LAYERS = [("layer1", 256, 56, 16), ("layer2", 512, 28, 32), ("layer3", 1024, 14, 64), ("layer4", 2048, 7, 128)]
ARCHS = ("resnext50_32x4d", "seresnext50_32x4d")


def se_launches(pkg, lib, B, HW, C, R, T16):
    """{kernel: (launch, bytes it must move)} over device tensors of one SE shape"""
    chk = pkg._lib.check
    st = lambda: torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(C + HW)
    act = lambda: torch.randn((B * HW, C), generator=g).to(T16).cuda()
    f32 = lambda *shape: torch.randn(shape, generator=g).cuda()
    u, sc, dy = act(), act(), act()
    y, gr, du = torch.empty_like(u), torch.empty_like(u), torch.empty_like(u)
    pooled, ds = f32(B, C), f32(B, C)
    w1, b1, w2, b2 = f32(R, C) / C ** 0.5, f32(R), f32(C, R) / R ** 0.5, f32(C)
    hidden, s, dpooled = torch.empty((B, R), device="cuda"), torch.empty((B, C), device="cuda"), torch.empty((B, C), device="cuda")
    dw1, db1, dw2, db2 = torch.empty_like(w1), torch.empty_like(b1), torch.empty_like(w2), torch.empty_like(b2)
    p = lambda t: t.data_ptr()
    n16, bc, cr = 2 * B * HW * C, 4 * B * C, 4 * C * R
    return {
        "mh_se_gate_fwd": (lambda: chk(lib.mh_se_gate_fwd(p(pooled), p(w1), p(b1), p(w2), p(b2), p(hidden), p(s), B, C, R, st()), "mh_se_gate_fwd"),
                           2 * cr + 2 * bc + 4 * (B * R + R + C)),
        "mh_se_apply_fwd": (lambda: chk(lib.mh_se_apply_fwd(p(u), p(s), p(sc), p(y), B, HW, C, st()), "mh_se_apply_fwd"), 3 * n16 + bc),
        "mh_se_apply_bwd_reduce": (lambda: chk(lib.mh_se_apply_bwd_reduce(p(dy), p(y), p(u), p(gr), p(ds), B, HW, C, st()), "mh_se_apply_bwd_reduce"),
                                   4 * n16 + bc),
        "mh_se_gate_bwd": (lambda: chk(lib.mh_se_gate_bwd(p(ds), p(s), p(hidden), p(pooled), p(w1), p(w2), p(dpooled), p(dw1), p(db1), p(dw2), p(db2),
                                                          B, C, R, 1.0, 0, st()), "mh_se_gate_bwd"), 4 * cr + 4 * bc + 4 * (B * R + R + C)),
        "mh_se_apply_bwd": (lambda: chk(lib.mh_se_apply_bwd(p(gr), p(s), p(dpooled), p(du), B, HW, C, st()), "mh_se_apply_bwd"), 2 * n16 + 2 * bc),
    }


def timed_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def se_share(path):
    """(SE kernels' share of the kernel time, {kernel: share}) from a rocprofv3 --stats kernel CSV"""
    total, per = 0.0, {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0.0)
            total += ns
            m = re.search(r"se_(?:gate|apply)_\w+?_kernel", name)
            if m:
                per[m.group(0)] = per.get(m.group(0), 0.0) + ns
    if not total:
        return None, {}
    return sum(per.values()) / total, {k: round(v / total, 4) for k, v in sorted(per.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--image-size", type=int, default=224)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--iters", type=int, default=20, help="launches between two events")
    ap.add_argument("--reps", type=int, default=7, help="timed windows per kernel")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed window of the whole-step comparison")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="per-kernel table only")
    ap.add_argument("--profile", type=int, default=0, help="N > 0: run N steps of seresnext50_32x4d and exit (for a profiler)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 --kernel-trace --stats CSV of a --profile run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seresnext_bench: needs the GPU (a CPU run measures nothing)")
    import multimodal_propaganda_meme_classification_amd as pkg
    B, S = args.batch, args.image_size
    T16 = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    lib = pkg._lib.load(args.dtype)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def step_fn(arch):
        torch.manual_seed(0)
        model = pkg.ResNetClassifier(num_labels=2, compute_dtype=args.dtype, arch=arch).cuda().train()
        pkg.flatten_parameters(model)
        opt = pkg.Adam(model.parameters(), lr=2e-5)
        g = torch.Generator().manual_seed(1)
        x, labels = torch.randn((B, 3, S, S), generator=g).cuda(), torch.randint(0, 2, (B,), generator=g).cuda()

        def step():
            opt.zero_grad()
            loss, _ = model(pixel_values=x, labels=labels)
            loss.backward()
            opt.step()
        return step

    if args.profile:
        step = step_fn("seresnext50_32x4d")
        for _ in range(args.profile):
            step()
        torch.cuda.synchronize()
        return

    for name, C, H, R in LAYERS:
        H = H * S // 224
        for kernel, (fn, nbytes) in se_launches(pkg, lib, B, H * H, C, R, T16).items():
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            t = [timed_ms(fn, args.iters) for _ in range(args.reps)]
            med = statistics.median(t)
            emit({"what": "kernel", "kernel": kernel, "layer": name, "batch": B, "HW": H * H, "C": C, "R": R, "median_us": round(med * 1e3, 2),
                  "min_max_us": [round(min(t) * 1e3, 2), round(max(t) * 1e3, 2)], "bytes": nbytes, "TBps": round(nbytes / med / 1e9, 3)})
        torch.cuda.empty_cache()
    summary = {"what": "summary", "dtype": args.dtype, "batch": B, "image_size": S, "device": torch.cuda.get_device_name(0),
               "torch": torch.__version__, "iters": args.iters, "reps": args.reps}

    if not args.no_step:
        steps = {arch: step_fn(arch) for arch in ARCHS}
        med = {a: [] for a in steps}
        for alt in range(args.alternations):
            for arch, step in steps.items():
                for _ in range(args.warmup):
                    step()
                torch.cuda.synchronize()
                per = []
                for _ in range(args.windows):
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        step()
                    torch.cuda.synchronize()
                    per.append((time.perf_counter() - t0) / args.steps)
                med[arch].append(statistics.median(per))
                emit({"what": "step_time", "arch": arch, "alternation": alt, "median_ms": round(med[arch][-1] * 1e3, 3),
                      "min_ms": round(min(per) * 1e3, 3), "max_ms": round(max(per) * 1e3, 3)})
        tx, tse = statistics.median(med["resnext50_32x4d"]), statistics.median(med["seresnext50_32x4d"])
        summary.update({"step": "forward + cross entropy + backward + Adam", "resnext50_32x4d_step_ms": round(tx * 1e3, 3),
                        "seresnext50_32x4d_step_ms": round(tse * 1e3, 3), "se_over_resnext": round(tse / tx, 3),
                        "se_minus_resnext_ms": round((tse - tx) * 1e3, 3), "seresnext50_32x4d_samples_per_s": round(B / tse, 1),
                        "resnext50_32x4d_samples_per_s": round(B / tx, 1),
                        "step_ms_spread": {a: [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)] for a, v in med.items()}})
    if args.kernel_stats:
        share, per = se_share(args.kernel_stats)
        summary.update({"se_kernels_share_of_kernel_time": None if share is None else round(share, 4), "se_kernels": per})
    emit(summary)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
