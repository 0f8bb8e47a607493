#!/usr/bin/env python3
"""ConvNeXt-tiny training throughput: convnext.ConvNeXtTiny.tower forward + backward, and the three depthwise kernels alone.

* the tower at --batch images of 224 x 224 (32), fp16 and bf16: --warmup steps, then --windows windows of --steps steps between two
  HIP events; images/s from the median window, library launches per step counted from the status checks of one step;
* mh_dwconv_nhwc, mh_dwconv_nhwc_dgrad (with the addend) and mh_dwconv_nhwc_wgrad (both of its kernels) at the four stage shapes of that
  batch: microseconds per call and the achieved bytes/s against the MINIMUM traffic of each (forward: x read + y written; dgrad: dy and
  addend read, dx written; wgrad: x and dy read once).  Every call of a timed pass works on its own set of buffers, enough sets to
  exceed the 256 MiB Infinity Cache, so the rate is an HBM rate and not a cache rate;
* the same depthwise weight gradient through torch (torch.nn.grad.conv2d_weight, channels-last fp16 / bf16) on the same GPU, as a
  comparison line -- informative, not a gate.

Prints one JSON line; --out also writes it to a file.  Launched by hand, never by the test suite.

  python tools/convnext_bench.py --out profiles/r06_convnext_train.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

STAGES = ((56, 96), (28, 192), (14, 384), (7, 768))          # (H = W, C) of convnext_tiny at 224 x 224
CACHE_BYTES = 600 << 20          # a timed pass touches at least this much: more than the Infinity Cache


def events_ms(fn, n):
    """milliseconds of n calls of fn(i) between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def median(v):
    return sorted(v)[len(v) // 2]


def tower_bench(dtype, B, warmup, steps, windows):
    from multimodal_propaganda_meme_classification_amd import convnext, ops
    net = convnext.ConvNeXtTiny(num_classes=0, compute_dtype=dtype, layer_scale=0.3).cuda()
    g = torch.Generator().manual_seed(1)
    x, r = torch.randn((B, 3, 224, 224), generator=g).cuda(), torch.randn((B, 768), generator=g).cuda()

    def step(_=0):
        (net.tower(x) * r).sum().backward()

    for _ in range(warmup):
        step()
    ms = [events_ms(step, steps) / steps for _ in range(windows)]
    calls = []
    orig = convnext.check

    def counting(status, what):
        calls.append(what)
        return orig(status, what)
    convnext.check = ops.check = counting
    try:
        step()
    finally:
        convnext.check = ops.check = orig
    torch.cuda.synchronize()
    launches = len(calls) + sum(1 for c in calls if c == "mh_dwconv_nhwc_wgrad")          # (its slab kernel and its finish kernel)
    finite = all(bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    return {"step_ms_median": round(median(ms), 3), "step_ms_windows": [round(v, 3) for v in ms], "images_per_s": round(B * 1000 / median(ms), 1),
            "library_launches_per_step": launches, "gradients_finite": finite}


def kernel_bench(dtype, B, passes):
    from multimodal_propaganda_meme_classification_amd import _lib, ops
    T16 = torch.float16 if dtype == "fp16" else torch.bfloat16
    lib, st = _lib.load(dtype), torch.cuda.current_stream().cuda_stream
    out = {}
    for H, C in STAGES:
        M, n = B * H * H, B * H * H * C
        sets = max(2, -(-CACHE_BYTES // (3 * n * 2)))
        g = torch.Generator().manual_seed(C)
        bufs = [[(torch.randn((M, C), generator=g) * 0.5).to(T16).cuda() for _ in range(2)] + [torch.empty((M, C), dtype=T16, device="cuda")]
                for _ in range(min(sets, 8))]
        while len(bufs) < sets:          # (distinct memory, same values)
            bufs.append([t.clone() for t in bufs[len(bufs) % 8]])
        wt = torch.randn((49, C), generator=g).cuda()
        bias = torch.randn(C, generator=g).cuda()
        dw, db = torch.empty((C, 1, 7, 7), device="cuda"), torch.empty(C, device="cuda")
        ws = torch.empty(ops.dwconv_wgrad_workspace_elems(B, H, H, C), device="cuda")

        def fwd(i):
            a, _, c = bufs[i % sets]
            _lib.check(lib.mh_dwconv_nhwc(a.data_ptr(), wt.data_ptr(), bias.data_ptr(), c.data_ptr(), B, H, H, C, 7, st), "mh_dwconv_nhwc")

        def dgrad(i):
            a, b, c = bufs[i % sets]
            _lib.check(lib.mh_dwconv_nhwc_dgrad(a.data_ptr(), wt.data_ptr(), b.data_ptr(), c.data_ptr(), B, H, H, C, 7, st), "mh_dwconv_nhwc_dgrad")

        def wgrad(i):
            a, b, _ = bufs[i % sets]
            _lib.check(lib.mh_dwconv_nhwc_wgrad(a.data_ptr(), b.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), B, H, H, C, 7, 1.0, 0, st),
                       "mh_dwconv_nhwc_wgrad")

        def torch_wgrad(i):
            a, b, _ = bufs[i % sets]
            xa = a.view(B, H, H, C).permute(0, 3, 1, 2)          # channels-last NCHW views of the same memory
            ya = b.view(B, H, H, C).permute(0, 3, 1, 2)
            torch.nn.grad.conv2d_weight(xa, (C, 1, 7, 7), ya, padding=3, groups=C)

        rec = {"rows": M, "buffer_sets": sets, "wgrad_workspace_MB": round(ws.numel() * 4 / 2 ** 20, 2)}
        for name, fn, nbytes in (("forward", fwd, 2 * n * 2), ("dgrad_addend", dgrad, 3 * n * 2), ("wgrad_and_finish", wgrad, 2 * n * 2),
                                 ("torch_conv2d_weight", torch_wgrad, 2 * n * 2)):
            try:
                fn(0), fn(1)          # warm-up: code object load (torch: its kernel search)
                us = median([events_ms(fn, sets) / sets * 1000 for _ in range(passes)])
                rec[name] = {"us": round(us, 2), "min_traffic_MB": round(nbytes / 2 ** 20, 2), "achieved_GB_per_s": round(nbytes / us / 1000, 1)}
            except Exception as e:          # (only the torch comparison can land here: a kernel library without this layout)
                if name != "torch_conv2d_weight":
                    raise
                rec[name] = {"failed": f"{type(e).__name__}: {e}"[:200]}
        out[f"{H}x{H}x{C}"] = rec
        del bufs
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5, help="steps per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3, help="timed passes over the buffer sets per kernel")
    ap.add_argument("--dtypes", default="fp16,bf16")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("convnext_bench: needs the GPU (a CPU run measures nothing)")
    import multimodal_propaganda_meme_classification_amd  # noqa: F401  (the built libraries: `python __graft_entry__.py` builds them)
    res = {"metric": "ConvNeXt-tiny tower forward + backward, images/s; depthwise kernels, us and bytes/s over minimum traffic", "batch": args.batch,
           "image": 224, "gpu": torch.cuda.get_device_name(0), "timing": f"HIP events, {args.warmup} warm-up steps, median of {args.windows} windows "
           f"x {args.steps} steps; kernels: median of {args.passes} passes over > 600 MB of distinct buffers"}
    for dtype in args.dtypes.split(","):
        res[dtype] = {"tower": tower_bench(dtype, args.batch, args.warmup, args.steps, args.windows)}
        torch.cuda.empty_cache()
        res[dtype]["dwconv_kernels"] = kernel_bench(dtype, args.batch, args.passes)
        if args.out:          # (kept after every dtype: a later failure loses nothing measured)
            with open(args.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
