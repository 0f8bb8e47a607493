#!/usr/bin/env python3
"""ResNeXt-50 32x4d on the MI355X: the grouped 3x3 kernels against the dense implicit-GEMM kernels, and the whole training step.

1. Per layer: the conv2 geometries of ResNeXt-50 at batch 32, 224 x 224 input (C = 128 @ 56^2, 256 @ 56^2 -> 28^2 and @ 28^2, 512 @ 28^2 -> 14^2
   and @ 14^2, 1024 @ 14^2 -> 7^2 and @ 7^2).  Each of mh_gconv_fwd / mh_gconv_dgrad / mh_gconv_wgrad (32 groups) is timed against mh_conv_fwd /
   mh_conv_dgrad / mh_conv_wgrad on the DENSE C -> C 3x3 of the same shape (launched as resnet._Conv launches them: split-K workspace where
   mh_conv_splitk takes one, the weight gradient's slabs without their finishing launch -- the grouped side includes its own).  HIP events
   around --iters launches, the two sides alternated --reps times, the median per side.  The condition has no margin: every grouped launch
   is faster than its dense counterpart ("grouped_faster").  bytes/s is the x + y traffic (what the layer must move) over the time.
2. Whole step: ResNetClassifier, batch 32, 224^2, fp16, forward + cross entropy + backward + Adam -- resnext50_32x4d against resnet50,
   alternated.  Reported, not gated.  --kernel-stats FILE: a ``rocprofv3 --kernel-trace --stats`` CSV of a ``--profile N`` run (a run of
   its own); the grouped kernels' share of the kernel time goes into the summary.

  python tools/resnext_bench.py --out profiles/r28_resnext.json
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
import torch.nn as nn  # noqa: E402

GROUPS = 32
LAYERS = [("layer1", 128, 56, 1), ("layer2.0", 256, 56, 2), ("layer2", 256, 28, 1), ("layer3.0", 512, 28, 2), ("layer3", 512, 14, 1),
          ("layer4.0", 1024, 14, 2), ("layer4", 1024, 7, 1)]


def layer_launches(pkg, lib, C, HW, stride, B, T16):
    """{direction: (dense launch, grouped launch)} over device tensors of one geometry"""
    R, chk = pkg.resnet, pkg._lib.check
    st = lambda: torch.cuda.current_stream().cuda_stream
    dense = R._Conv(nn.Conv2d(C, C, 3, stride=stride, padding=1, bias=False))
    Ho, Wo = dense.out_hw(HW, HW)
    M, Mi = B * Ho * Wo, B * HW * HW
    g = torch.Generator().manual_seed(C + HW)
    x = torch.randn((Mi, C), generator=g).to(T16).cuda()
    dy = torch.randn((M, C), generator=g).to(T16).cuda()
    y, dx = torch.empty((M, C), dtype=T16, device="cuda"), torch.empty((Mi, C), dtype=T16, device="cuda")
    part = torch.empty((2, C, (M + 127) // 128), device="cuda")
    geom = dense.geom(B, HW, HW)
    wd = (torch.randn((C, C, 3, 3), generator=g) * 0.05).cuda()
    wkd = torch.empty((C, dense.ldk), dtype=T16, device="cuda")
    chk(lib.mh_conv_weight_pack(wd.data_ptr(), wkd.data_ptr(), C, C, 3, 3, C, dense.ldk, st()), "mh_conv_weight_pack")
    spf, spd = int(lib.mh_conv_splitk(geom, 0)), int(lib.mh_conv_splitk(geom, 1))
    wsf = torch.empty((spf, M, C), device="cuda") if spf > 1 else None
    wsd = torch.empty((spd, Mi, C), device="cuda") if spd > 1 else None
    spw = dense._wgrad_split(lib, M, R.WGRAD_TILES)
    slabs = torch.empty((spw, C, dense.ldk), device="cuda")
    assert R.dgrad_route(dense, HW, HW, R.TowerOptions()) == R.IMPLICIT
    wg = (torch.randn((C, C // GROUPS, 3, 3), generator=g) * 0.05).cuda()
    wkg = torch.empty(int(lib.mh_gconv_packed_elems(C, GROUPS)), dtype=T16, device="cuda")
    chk(lib.mh_gconv_weight_pack(wg.data_ptr(), wkg.data_ptr(), C, GROUPS, st()), "mh_gconv_weight_pack")
    dwg = torch.empty_like(wg)
    wsg = torch.empty(int(lib.mh_gconv_wgrad_workspace_elems(geom, GROUPS)), device="cuda")
    p = lambda t: None if t is None else t.data_ptr()
    return dict(bytes=2 * (Mi + M) * C, rows=(Mi, M), dense_splitk=dict(fwd=spf, dgrad=spd, wgrad=spw), launches={
        "fwd": (lambda: chk(lib.mh_conv_fwd(p(x), p(wkd), p(y), p(part), p(wsf), geom, st()), "mh_conv_fwd"),
                lambda: chk(lib.mh_gconv_fwd(p(x), p(wkg), p(y), p(part), geom, GROUPS, st()), "mh_gconv_fwd")),
        "dgrad": (lambda: chk(lib.mh_conv_dgrad(p(dy), p(wkd), p(dx), p(wsd), geom, None, st()), "mh_conv_dgrad"),
                  lambda: chk(lib.mh_gconv_dgrad(p(dy), p(wkg), p(dx), geom, GROUPS, st()), "mh_gconv_dgrad")),
        "wgrad": (lambda: chk(lib.mh_conv_wgrad(p(dy), p(x), p(slabs), spw, 1.0, geom, st()), "mh_conv_wgrad"),
                  lambda: chk(lib.mh_gconv_wgrad(p(dy), p(x), p(dwg), p(wsg), 0, 1.0, geom, GROUPS, st()), "mh_gconv_wgrad")),
    })


def timed_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def grouped_share(path):
    """(grouped kernels' share of the kernel time, their names) from a rocprofv3 --stats kernel CSV"""
    total = grouped = 0.0
    names = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0.0)
            total += ns
            if "gconv_" in name:
                grouped += ns
                names.append(re.search(r"gconv_\w+", name).group(0))
    return (grouped / total if total else None), sorted(set(names))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--image-size", type=int, default=224)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--iters", type=int, default=20, help="launches between two events")
    ap.add_argument("--reps", type=int, default=7, help="alternations of the two sides")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed window of the whole-step comparison")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="per-layer comparison only")
    ap.add_argument("--profile", type=int, default=0, help="N > 0: run N steps of resnext50_32x4d and exit (for a profiler)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 --kernel-trace --stats CSV of a --profile run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resnext_bench: needs the GPU (a CPU run measures nothing)")
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
        step = step_fn("resnext50_32x4d")
        for _ in range(args.profile):
            step()
        torch.cuda.synchronize()
        return

    all_faster = True
    for name, C, HW, stride in LAYERS:
        HW = HW * S // 224
        L = layer_launches(pkg, lib, C, HW, stride, B, T16)
        for direction, (dense, grouped) in L["launches"].items():
            for fn in (dense, grouped):
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            td, tg = [], []
            for _ in range(args.reps):
                td.append(timed_ms(dense, args.iters))
                tg.append(timed_ms(grouped, args.iters))
            d, g_ = statistics.median(td), statistics.median(tg)
            faster = max(tg) < min(td) if g_ < d else False
            all_faster &= g_ < d
            emit({"what": "layer", "layer": name, "C": C, "input": HW, "stride": stride, "batch": B, "direction": direction,
                  "dense_ms": round(d, 4), "grouped_ms": round(g_, 4), "dense_over_grouped": round(d / g_, 2), "grouped_faster": g_ < d,
                  "every_rep_faster": faster, "dense_min_max_ms": [round(min(td), 4), round(max(td), 4)],
                  "grouped_min_max_ms": [round(min(tg), 4), round(max(tg), 4)], "dense_splitk": L["dense_splitk"][direction],
                  "xy_bytes": L["bytes"], "grouped_xy_GBps": round(L["bytes"] / g_ / 1e6, 1), "dense_xy_GBps": round(L["bytes"] / d / 1e6, 1)})
        del L
        torch.cuda.empty_cache()
    summary = {"what": "summary", "dtype": args.dtype, "batch": B, "image_size": S, "groups": GROUPS, "every_grouped_launch_faster": all_faster,
               "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": args.iters, "reps": args.reps}

    if not args.no_step:
        steps = {arch: step_fn(arch) for arch in ("resnet50", "resnext50_32x4d")}
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
        t50, tx = statistics.median(med["resnet50"]), statistics.median(med["resnext50_32x4d"])
        summary.update({"step": "forward + cross entropy + backward + Adam", "resnet50_step_ms": round(t50 * 1e3, 3),
                        "resnext50_32x4d_step_ms": round(tx * 1e3, 3), "resnext_over_resnet50": round(tx / t50, 3),
                        "resnext50_32x4d_samples_per_s": round(B / tx, 1), "resnet50_samples_per_s": round(B / t50, 1)})
    if args.kernel_stats:
        share, names = grouped_share(args.kernel_stats)
        summary.update({"grouped_kernels_share_of_kernel_time": None if share is None else round(share, 4), "grouped_kernels": names})
    emit(summary)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
