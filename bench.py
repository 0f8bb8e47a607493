#!/usr/bin/env python
"""Headline benchmark: memes/sec of one full fine-tune step (forward + cross-entropy + backward +
Adam) of the Subtask-2C dual encoder, ViT-B/16 + BERT-base(V=64000), 224x224 + 128 tokens, batch 32
per GPU (BASELINE.json configs[2]; configs[3] = the same per-GPU work on N GPUs, weak scaling).

    python bench.py --gpus 1 --steps 20 --warmup 5
    python bench.py --full          # + roofline, the secondary lines, cpu_baseline
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Prints ONE JSON line (rank 0).  Inputs are synthetic and already resident in HBM when the timed
region starts; a "step" is one pass of the hot path over one batch.
A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the line: nothing
else.  Whatever takes runs of its own comes with --full:
`roofline` prices the dominant kernel (the grouped bf16 MFMA GEMM with the largest share of the
step) from HIP events recorded around each of its launches on the launch stream, in an
instrumented eager replay of the same prepared launches right after the timed region.
`value_<variant>` / `ms_per_step_<variant>` (single GPU, config 3) time the same step under other
switches (other storage type, all-ones masks, dense text rows, unguarded / clipped / dropout
variants, one resident batch) and BASELINE configs 5 and 2.
`cpu_baseline` times the CPU oracle (oracle/meme_oracle.py, a port -- the reference itself cannot
run here) on a bounded sample of the same workload on this host's cores.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FLOP_PER_MEME = {3: 172.42e9,      # fwd+bwd algorithmic FLOPs per meme, config 3
                 5: 1628.9e9}      # config 5: CLIP ViT-L/14@336 (577 tokens) + BERT-large at S = 256
MFMA_PEAK_TFLOPS = 2500.0         # dense bf16/fp16 MFMA peak, MI355X_MICROARCH.md "Chip-level parameters"
DUMP_LIMIT_BYTES = 64 << 20       # --dump-outputs: all arrays together
DUMP_PER_PARAM = 8192             # --dump-outputs: elements sampled from each parameter tensor (seeded, the same every run)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32, help="memes per GPU")
    ap.add_argument("--seq", type=int, default=0, help="text tokens (default: 128 for config 3, 256 for config 5)")
    ap.add_argument("--config", type=int, choices=(2, 3, 5), default=3,
                    help="BASELINE.json configuration: 3 = ViT-B/16 + BERT-base (the headline metric), "
                         "5 = CLIP ViT-L/14@336 + BERT-large, seq 256, 2 = Subtask-2B ResNet-50 image-only (single GPU)")
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of hipGraph replay")
    ap.add_argument("--full", action="store_true",
                    help="also measure what takes runs of its own: the dominant kernel's roofline (instrumented replay), the "
                         "secondary lines and the CPU baseline.  Without it a run prints the headline figure only")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--cpu-batch", type=int, default=32)
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: skip the secondary lines (other storage type, all-ones masks, dense text rows, unguarded / "
                         "clipped / dropout variants, configs 5 and 2)")
    ap.add_argument("--batches", type=int, default=8,
                    help="distinct synthetic batches resident in HBM, loaded in turn (one device-to-device copy per step inside the timed "
                         "region): other token ids, other ragged masks every step, as a DataLoader would hand over; 1 = replay one batch")
    ap.add_argument("--unguarded", action="store_true", help="A/B: fp16 without overflow protection (skip_nonfinite=False, no loss scaler)")
    ap.add_argument("--clip", type=float, default=0.0, help="A/B: max_grad_norm (the Trainer / Kevin variants clip at 1.0)")
    ap.add_argument("--reference-dropout", action="store_true", help="A/B: BERT 0.1 / 0.1 + head Dropout(0.3), as the reference trains")
    ap.add_argument("--tiny", action="store_true", help="tiny model (debug only; not a bench line)")
    ap.add_argument("--no-overlap-wgrad", action="store_true", help="A/B: weight-gradient GEMMs on the main stream")
    ap.add_argument("--no-overlap-opt", action="store_true", help="A/B: whole Adam update after the backward")
    ap.add_argument("--force-ddp", action="store_true",
                    help="debug: run the data-parallel code path (segmented graphs, RCCL all-reduce) on a 1-rank group")
    ap.add_argument("--ddp-mode", choices=("stream", "segments", "graph"), default=None,
                    help="data-parallel schedule (default: MEMEHIP_DDP_MODE or 'segments'): one hipGraph per backward segment, or forward "
                         "graph + stream-ordered eager backward with the all-reduces behind a fence stream")
    ap.add_argument("--ddp-compress", choices=("none", "bf16"), default="none",
                    help="wire format of the gradient exchange.  none (default): fp32 RCCL all-reduce -- the exact sum, what the headline and the "
                         "scaling numbers are quoted on.  bf16: all-to-all + all-gather in bf16 with fp32 accumulation on receipt (half the bytes "
                         "per link, every gradient element rounded twice): an option for link-bound runs, reported as such in the JSON line "
                         "(`ddp_wire`)")
    ap.add_argument("--dense-text", action="store_true",
                    help="A/B: compute every padded text position like the reference does (default: padding-free text tower)")
    ap.add_argument("--full-masks", action="store_true", help="all-ones attention masks (SURVEY 8d's second input variant)")
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="fp16",
                    help="16-bit storage / MFMA operand type of the towers (same kernels, same MFMA peak).  Default fp16: the "
                         "storage type that meets north_star's 1e-3 logit tolerance (and the reference's own AMP arithmetic, "
                         "Multimodal_example_task2C.py:60-64); the bf16 build is timed beside it with --full (value_bf16)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (loss, correct count, logits, a seeded sample "
                         "of every updated parameter) as DIR/<name>.npy in float32, to compare two builds output for output")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if a.seq <= 0:
        a.seq = 256 if a.config == 5 else 128
    return a


def make_config(pkg, args):
    if args.tiny:
        return pkg.ModelConfig(text=pkg.TextConfig(vocab_size=512, hidden=128, layers=2, heads=2, intermediate=256, max_position=64),
                               image=pkg.ImageConfig(image_size=32, hidden=128, layers=2, heads=2, intermediate=256), proj=128)
    if args.config == 5:
        return pkg.ModelConfig(
            text=pkg.TextConfig(vocab_size=30522, hidden=1024, layers=24, heads=16, intermediate=4096),
            image=pkg.ImageConfig(image_size=336, patch=14, hidden=1024, layers=24, heads=16, intermediate=4096, ln_eps=1e-5,
                                  act="quick_gelu", pre_ln=True, patch_bias=False))
    return pkg.ModelConfig()            # config 3


def synthetic_batch(cfg, batch, seq, seed, device, full_masks=False):
    """image ~ N(0,1); ids ~ U{5..V-1}, id[:,0] = CLS-like, PAD 0; ragged masks."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    ic = cfg.image
    image = torch.randn((batch, ic.channels, ic.image_size, ic.image_size), generator=g)
    text = torch.randint(5, cfg.text.vocab_size, (batch, seq), generator=g, dtype=torch.int64)
    lens = torch.randint(min(8, seq), seq + 1, (batch,), generator=g)
    if full_masks:
        lens = torch.full((batch,), seq)
    mask = (torch.arange(seq)[None] < lens[:, None]).to(torch.int64)
    text = text * mask
    text[:, 0] = 2
    labels = (torch.rand((batch,), generator=g) < 0.28).to(torch.int64)
    return [t.to(device) for t in (text, image, mask, labels)]


def cpu_model_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(batch, seq, tiny, warm=3, timed=5, config=3):
    """Oracle fine-tune step (fp32, eager PyTorch CPU, dropout 0) on a bounded sample: BASELINE.md section 3 --
    the same synthetic batch shape as the GPU run (batch 32), >= 3 warm-up + >= 5 timed steps, median."""
    from oracle import meme_oracle as O
    cfg = O.tiny_config("cls") if tiny else (O.config5("cls") if config == 5 else O.config3("cls"))
    torch.set_num_threads(min(16, os.cpu_count() or 1))      # the GPU box's CPU share for one GPU
    threads = torch.get_num_threads()
    params = O.init_params(cfg, seed=0)
    text, image, mask, labels = O.synthetic_batch(cfg, batch, seq, seed=1234)
    st = O.AdamState()
    for _ in range(warm):
        params, *_ = O.train_step(params, st, text, image, mask, labels, cfg, lr=2e-5)
    times = []
    for _ in range(timed):
        t0 = time.perf_counter()
        params, *_ = O.train_step(params, st, text, image, mask, labels, cfg, lr=2e-5)
        times.append(time.perf_counter() - t0)
    times.sort()
    t = times[len(times) // 2]
    return {"value": round(batch / t, 3), "unit": "memes/s", "cores": threads, "kind": "port", "cpu_model": cpu_model_name(),
            "sample": f"oracle train_step (fwd+CE+bwd+Adam, fp32, eager PyTorch CPU) on the GPU run's synthetic batch shape: "
                      f"batch {batch}, seq {seq}; {warm} warm-up + {timed} timed steps, median {t:.2f} s/step "
                      f"(min {times[0]:.2f}, max {times[-1]:.2f}) on {threads} threads"}


def opt_kwargs(args, unguarded=None, clip=None):
    kw = {}
    if (args.unguarded if unguarded is None else unguarded):
        kw["skip_nonfinite"] = False
    c = args.clip if clip is None else clip
    if c and c > 0:
        kw["max_grad_norm"] = float(c)
    return kw


def make_batches(cfg, args, device, rank=0, full_masks=None, n=None):
    fm = args.full_masks if full_masks is None else full_masks
    return [synthetic_batch(cfg, args.batch, args.seq, seed=1234 + rank + 7919 * k, device=device, full_masks=fm)
            for k in range(max(1, args.batches if n is None else n))]


def param_sample(module):
    """A fixed, seeded sample of every parameter of ``module`` (name order, at most DUMP_PER_PARAM elements each), concatenated
    into one float32 vector: the same elements on every run and for every build whose parameters have the same names and shapes."""
    g = torch.Generator(device="cpu").manual_seed(20240917)
    parts = []
    for _, p in sorted(module.named_parameters(), key=lambda kv: kv[0]):
        flat = p.detach().reshape(-1)
        if flat.numel() > DUMP_PER_PARAM:
            idx = torch.randint(0, flat.numel(), (DUMP_PER_PARAM,), generator=g).sort().values
            flat = flat[idx.to(flat.device)]
        parts.append(flat.float().cpu())
    return torch.cat(parts)


def dump_outputs(dirname, arrays):
    """Write ``{name: tensor}`` as dirname/<name>.npy, float32, at most DUMP_LIMIT_BYTES in all."""
    import numpy as np
    host = {k: np.ascontiguousarray(v.detach().float().cpu().numpy(), dtype=np.float32) for k, v in arrays.items()}
    total = sum(a.nbytes for a in host.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit(f"--dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES}-byte limit")
    os.makedirs(dirname, exist_ok=True)
    for k, a in host.items():
        np.save(os.path.join(dirname, f"{k}.npy"), a)


def run_steps(step, batches, n, start=0):
    out = None
    for i in range(n):
        step.load_batch(*batches[(start + i) % len(batches)])
        out = step.step()
    return out


def timed_variant(pkg, args, device, dtype=None, full_masks=None, dense_text=None, unguarded=None, clip=None, reference_dropout=None,
                  config=None, n_batches=None):
    """One more single-GPU measurement of the same step under a different switch: returns (memes/s, ms/step)."""
    import copy
    a = copy.copy(args)
    if config is not None:
        a.config = config
        a.seq = 256 if config == 5 else 128
    cfg = make_config(pkg, a)
    cfg.compute_dtype = dtype or args.dtype
    cfg.pack_text = not (args.dense_text if dense_text is None else dense_text)
    if (args.reference_dropout if reference_dropout is None else reference_dropout):
        cfg.with_reference_dropout()
    model = pkg.MultimodalClassifier.from_config(cfg, device=device, seed=0)
    model.train()
    opt = pkg.Adam(model.parameters(), lr=2e-5, model=model, **opt_kwargs(args, unguarded, clip))
    step = pkg.GraphedStep(model, opt, a.batch, a.seq, use_graph=not args.no_graph,
                           overlap_wgrad=not args.no_overlap_wgrad, overlap_optimizer=not args.no_overlap_opt)
    batches = make_batches(cfg, a, device, full_masks=full_masks, n=n_batches)
    run_steps(step, batches, max(args.warmup, 1))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss, _ = run_steps(step, batches, args.steps, start=max(args.warmup, 1))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    # the variant has to be TRAINING, not just running: a finite loss in the range a 2-class cross-entropy of a freshly initialised
    # model under a handful of Adam steps can have, finite weights, no step skipped by the overflow guard on these inputs
    final = float(loss)
    if not (0.0 < final < 3.0) or not bool(torch.isfinite(model.flat_params).all()):
        raise SystemExit(f"bench variant {dict(dtype=dtype, config=config, clip=clip)}: loss {final} / non-finite weights -- not a valid measurement")
    step.close()
    del step, opt, model, batches
    torch.cuda.empty_cache()
    return a.batch * args.steps / dt, dt / args.steps * 1e3


def bench_config2(args, dump_dir=None):
    """BASELINE.json configs[1]: Subtask 2B, ResNet-50 image-only, 224x224 synthetic, batch 32, one MI355X: images/s of one
    fine-tune step (forward + cross-entropy + backward + fused Adam) through the Trainer-protocol module, replayed as a hipGraph."""
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    import multimodal_propaganda_meme_classification_amd as pkg
    model = pkg.ResNetClassifier(num_labels=2, compute_dtype=args.dtype).to(device)
    pkg.flatten_parameters(model)
    model.train()
    # fp16 activations: the all-or-nothing overflow check (global norm, then the update) -- skip_nonfinite=True
    opt = pkg.Adam(model.parameters(), lr=2e-5, skip_nonfinite=(args.dtype == "fp16" and not args.unguarded))
    g = torch.Generator().manual_seed(1234)
    nb = max(1, args.batches)
    images = [torch.randn((args.batch, 3, 224, 224), generator=g).to(device) for _ in range(nb)]
    labelss = [(torch.rand((args.batch,), generator=g) < 0.28).long().to(device) for _ in range(nb)]
    image, labels = images[0].clone(), labelss[0].clone()          # the graph's static input buffers
    loss_buf = torch.zeros((), device=device)
    turn = [0]
    last = {}                       # the logits of the last launch (a graph output: replay rewrites them in place)

    def launches():                 # everything of a step that is a device launch (capturable)
        opt.zero_grad()
        loss, logits = model(pixel_values=image, labels=labels)
        loss.backward()
        opt.launch()
        loss_buf.copy_(loss.detach())
        last["logits"] = logits.detach()

    def one_step():
        k = turn[0] % nb
        turn[0] += 1
        image.copy_(images[k], non_blocking=True)
        labels.copy_(labelss[k], non_blocking=True)
        opt._step += 1              # the per-step scalars (step count, bias corrections, lr) are written OUTSIDE the graph,
        opt._write_hyper()          # as GraphedStep does: captured inside they would freeze at their capture-time values
        (graph.replay if graph is not None else launches)()

    graph = None
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.zero_grad()
        loss0, _ = model(pixel_values=image, labels=labels)
        loss0.backward()
        opt.step()                  # binds the optimizer to the flat buffers (eager)
        one_step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    if not args.no_graph:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            launches()
    run = one_step
    for _ in range(max(args.warmup, 1)):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        run()
    t_issue = time.perf_counter() - t0
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    value = args.batch * args.steps / dt
    if dump_dir:
        dump_outputs(dump_dir, {"loss": loss_buf.reshape(1), "logits": last["logits"], "params_sample": param_sample(model)})
    flop_per_image = 24.5e9          # fwd + bwd, BASELINE.md section 2
    out = {"metric": "images/sec (fine-tune step) ResNet-50 224x224 bs=32 (BASELINE configs[1], Subtask 2B)", "value": round(value, 2),
           "unit": "images/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3),
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
           "config": {"workload": f"Subtask-2B fine-tune step: torchvision-topology ResNet-50 (25.6 M parameters), 3x224x224, batch {args.batch}, "
                                  "fwd+CE+bwd+Adam, train-mode BatchNorm, random-init weights; convolutions = implicit MFMA GEMM on NHWC (no im2col panel), BatchNorm statistics from the conv epilogue; "
                                  f"{nb} resident batches in turn",
                      "global_batch": args.batch, "image": "3x224x224", "parallelism": "dp1",
                      "launch": "eager" if args.no_graph else "hipGraph", "final_loss": round(float(loss_buf), 5),
                      "host_issue_ms_per_step": round(t_issue / args.steps * 1e3, 3)},
           "roofline": {"bound": "mfma", "kernel": "whole step (implicit conv GEMMs + BatchNorm passes)",
                        "achieved": round(flop_per_image * value / 1e12, 1), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(flop_per_image * value / (MFMA_PEAK_TFLOPS * 1e12), 4), "traffic": None}}
    del graph, opt, model, last
    torch.cuda.empty_cache()
    return out


def gemm_roofline(plan, args, value, world, dyn_scale):
    """`roofline` of the dominant kernel: an instrumented eager replay of the step's prepared launches on the launch stream.
    ``dyn_scale`` = live / allocated text rows (the text launches are sized for batch*seq rows and clamp on the device)."""
    stream = torch.cuda.current_stream().cuda_stream
    tags = ("gemm<0,0>", "gemm<0,1>", "gemm<1,1>")
    per_tag = {}
    for tag in tags:
        recs = []
        for _ in range(3):
            plan.fwd.run_timed(stream, tag, recs, dyn_scale)
            plan.loss.run(stream)
            for seg in plan.bwd:
                seg.run_timed(stream, tag, recs, dyn_scale)
        torch.cuda.synchronize()
        ms = [e0.elapsed_time(e1) for e0, e1, _ in recs]
        per_tag[tag] = dict(launches=len(recs) // 3, total_ms=sum(ms) / 3, flops=sum(w for _, _, w in recs) / 3)
    dom = max(per_tag, key=lambda k: per_tag[k]["total_ms"])
    d = per_tag[dom]
    achieved = d["flops"] / (d["total_ms"] * 1e-3) / 1e12
    # HBM bytes per launch of that kernel: from the committed rocprofv3 --pmc passes (FETCH_SIZE x2 + WRITE_SIZE,
    # tools/traffic_from_pmc.py); PMC counters cannot be read from inside the process
    traffic = None
    traffic_src = None
    try:
        tpath = next(pth for pth in (os.path.join(ROOT, "profiles", f) for f in ("r04_traffic.json", "r03_traffic.json", "r02_traffic.json", "r01_traffic.json"))
                     if os.path.exists(pth))
        traffic_src = os.path.relpath(tpath, ROOT)
        tj = json.load(open(tpath))["kernels"]
        pref = f"gemm_kernel<{dom[5]}, {dom[7]},"
        hit = [v for k, v in tj.items() if k.startswith(pref)]
        if hit and not args.tiny and args.batch == 32 and args.config == 3:
            traffic = max(hit, key=lambda v: v["launches_sampled"])["hbm_bytes_per_launch"]
    except Exception:
        traffic = None
    flop_per_meme = FLOP_PER_MEME[args.config] if not args.tiny else plan.gemm_flops / args.batch
    # FLOPs actually executed: the GEMM work of the text rows that were packed away is not counted
    flop_exec_per_meme = flop_per_meme - plan.gemm_flops_dyn * (1.0 - dyn_scale) / args.batch
    return {"bound": "mfma", "kernel": f"gemm_kernel{dom[4:]} (grouped {args.dtype} MFMA GEMM)",
            "achieved": round(achieved, 1), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(achieved / MFMA_PEAK_TFLOPS, 4), "traffic": traffic,
            "traffic_source": (f"{traffic_src}: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command "
                               "(FETCH x2, KiB -> bytes; tools/collect_profiles.sh), per launch of this kernel; "
                               "PMC counters cannot be read from inside the process") if traffic is not None else None,
            "method": "HIP events around every launch of the kernel on its launch stream, in an eager one-stream "
                      "replay of the step's prepared launches right after the timed region (3 replays averaged)",
            "launches_per_step": d["launches"], "avg_launch_us": round(d["total_ms"] / d["launches"] * 1e3, 2),
            "flops_per_launch": round(d["flops"] / d["launches"]),
            "all_gemm_kernels": {k: {"ms_per_step": round(v["total_ms"], 3),
                                     "tflops": round(v["flops"] / (v["total_ms"] * 1e-3) / 1e12, 1)}
                                 for k, v in per_tag.items()},
            "step_mfma_frac": round(flop_exec_per_meme * value / world / (MFMA_PEAK_TFLOPS * 1e12), 4)}


def main():
    args = parse()
    if args.config == 2:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs an MI355X (no CPU fallback for the product path)")
        print(json.dumps(bench_config2(args, dump_dir=args.dump_outputs)), flush=True)
        return
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.gpus > 1 and world == 1:
        raise SystemExit("launch N>1 with: python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback for the product path)")
    if os.environ.get("MEMEHIP_BENCH_SHARE_DEVICE") == "1":      # rehearsal of the N > 1 path on a 1-GPU box (with gloo)
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    import torch.distributed as dist
    if world > 1 or args.force_ddp:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29577")
        if world > 1:
            backend = os.environ.get("MEMEHIP_DIST_BACKEND", "nccl")       # "nccl" is RCCL on ROCm
            if backend == "nccl":
                dist.init_process_group("nccl", device_id=device)
            else:
                dist.init_process_group(backend)
        else:
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=device)

    import multimodal_propaganda_meme_classification_amd as pkg
    from multimodal_propaganda_meme_classification_amd import ddp

    cfg = make_config(pkg, args)
    cfg.compute_dtype = args.dtype
    cfg.pack_text = not args.dense_text
    if args.reference_dropout:
        cfg.with_reference_dropout()
    model = pkg.MultimodalClassifier.from_config(cfg, device=device, seed=0)
    model.train()
    reducer = None
    if world > 1 or args.force_ddp:
        ddp.broadcast_parameters(model.flat_params)
        model.mark_weights_changed()
        compress = None if args.ddp_compress == "none" else args.ddp_compress
        if compress and world > 1 and (args.ddp_mode or os.environ.get("MEMEHIP_DDP_MODE", "segments")) == "graph":
            #  the captured form of the compressed exchange -- private comm stream, staging buffers, all_to_all inside a hipGraph --
            # has only ever run on a 1-rank group, where nothing is compressed, and cannot be rehearsed on a 1-GPU box: refuse it
            raise SystemExit("--ddp-mode graph with --ddp-compress bf16 is not supported on more than one rank (never exercised at W > 1)")
        reducer = ddp.GradientReducer(model.flat_grads, compress=compress)
    opt = pkg.Adam(model.parameters(), lr=2e-5, model=model, **opt_kwargs(args))
    step = pkg.GraphedStep(model, opt, args.batch, args.seq, use_graph=not args.no_graph, reducer=reducer,
                           overlap_wgrad=not args.no_overlap_wgrad, overlap_optimizer=not args.no_overlap_opt, ddp_mode=args.ddp_mode)
    if reducer is not None:
        end = ddp.check_bucket_cover(step.plan.bucket_after, model.layout.n_total)
        assert end == model.layout.spec["bert.embeddings.token_type_embeddings.weight"].offset, end
    batches = make_batches(cfg, args, device, rank=rank)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    run_steps(step, batches, max(args.warmup, 1))       # >= 1: the first call captures the graph(s)
    barrier()
    t0 = time.perf_counter()
    loss, _ = run_steps(step, batches, args.steps, start=max(args.warmup, 1))
    barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t)
    final_loss = float(loss)
    ms_per_step = dt / args.steps * 1e3
    if args.dump_outputs and rank == 0:      # before the roofline replay below rewrites the step's buffers
        dump_outputs(args.dump_outputs, {"loss": loss, "ncorrect": step.plan.buf["ncorrect"], "logits": step.plan.buf["logits"],
                                         "params_sample": param_sample(model)})
    value = args.batch * world * args.steps / dt

    out = None
    if rank == 0:
        plan = step.plan
        # padding-free text tower: the text launches are sized for batch*seq rows and clamp to the live rows on the device
        max_rows = args.batch * args.seq
        live_rows = int(plan.buf["pk.n_rows"]) if plan.packed else max_rows
        roofline = gemm_roofline(plan, args, value, world, live_rows / max_rows) if args.full else None
        out = {
            "metric": ("memes/sec (fine-tune step) ViT-B/16+BERT-base bs=32, 1/2/4/8 MI355X" if args.config == 3 else
                       "memes/sec (fine-tune step) CLIP ViT-L/14@336 + BERT-large seq=256 (BASELINE configs[4])"),
            "value": round(value, 2), "unit": "memes/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.dtype, "data": "synthetic",
            # wire format of the data-parallel gradient exchange, next to `value`: fp32 = exact RCCL all-reduce (default)
            "ddp_wire": (None if reducer is None else ("bf16 all-to-all + fp32 accumulation + bf16 all-gather" if reducer.compress else "fp32 all-reduce")),
            "config": {"workload": ("Subtask-2C fine-tune step: ViT-B/16 (224x224, 197 tokens) + BERT-base (V=64000, "
                                    if args.config == 3 else
                                    "Subtask-2C fine-tune step: CLIP ViT-L/14 (336x336, 577 tokens, quick-GELU, pre-LN) + "
                                    "BERT-large (V=30522, ") +
                                   f"S={args.seq}) late-fusion, fwd+CE+bwd+Adam, batch {args.batch}/GPU, random-init weights"
                                   + (" [TINY DEBUG MODEL]" if args.tiny else ""),
                       "global_batch": args.batch * world, "seq_len": args.seq,
                       "image": f"3x{cfg.image.image_size}x{cfg.image.image_size}",
                       "params": model.layout.n_total, "parallelism": f"dp{world}",
                       "launch": "eager" if args.no_graph else ("hipGraph" if reducer is None else
                                                                ("ONE hipGraph for the whole step, the RCCL all-reduce of every completed gradient slice captured in it"
                                                                 if step.ddp_graph else
                                                                 "forward hipGraph + stream-ordered backward launches, RCCL all-reduce per completed gradient slice"
                                                                 if step.ddp_stream else "hipGraph per backward segment + RCCL all-reduce")),
                       "kernel_launches_per_step": plan.n_launches, "final_loss": round(final_loss, 5),
                       "masks": "all ones" if args.full_masks else "ragged, valid length ~ U{8..seq} (SURVEY 8d)",
                       "batches": f"{len(batches)} distinct synthetic batches resident in HBM, loaded in turn (one device-to-device copy of "
                                  "ids / mask / pixels / labels per step, inside the timed region)",
                       "overflow_protection": ("none (skip_nonfinite=False)" if opt.skip_nonfinite is False else
                                               ("all-or-nothing: global gradient norm before any update" if not step.opt_in_bwd and reducer is None else
                                                "guarded optimizer-in-backward updates") +
                                               (f" + dynamic loss scale on the device (GradScaler rule; scale now {step.scaler.get_scale():g} x "
                                                f"{cfg.stream_scale:g})" if step.scaler is not None else "")),
                       "dropout": "BERT 0.1 / 0.1, head 0.3 (reference)" if args.reference_dropout else "0 (BASELINE.md section 3)",
                       "clip": args.clip if args.clip > 0 else None,
                       "optimizer": f"Adam lr 2e-5, dense semantics over all {model.layout.n_total / 1e6:.1f} M parameters every step (word-embedding rows "
                                    "that never received a gradient are the identity under Adam and are skipped: bit-identical)",
                       "text_rows": (f"padding-free: {live_rows} of {max_rows} token rows live on rank 0 (attention_mask != 0), "
                                     "padded positions never computed") if plan.packed else f"dense: all {max_rows} rows computed"},
            **({"roofline": roofline} if roofline is not None else {}),
            # the tolerance every storage type is held to on THIS configuration (config 3, batch 32) by the GPU suite
            "parity": {"fp16": {"tol_logits": 1e-3, "test": "tests/test_round2_gpu.py::test_config3_batch32_matches_the_fixture[fp16]"},
                       "bf16": {"tol_logits": 8e-3, "test": "tests/test_round2_gpu.py::test_config3_batch32_matches_the_fixture[bf16]"}},
        }
        if args.full and world == 1 and not args.force_ddp and not args.no_extras and not args.tiny and args.config == 3:
            # secondary lines, same K / W, same batch: the other 16-bit storage type (fp16 meets north_star's 1e-3 on the
            # logits, see "parity"), SURVEY 8d's all-ones masks, the reference's dense text rows; fp16 WITHOUT overflow protection
            # (round 2's headline mode), the Trainer / Kevin clip at 1.0 (needs the global norm: no optimizer-in-backward), the
            # reference's dropout probabilities, ONE replayed batch (round 2's methodology); then BASELINE configs 5 and 2
            step.close()
            del step, opt, model, plan, batches
            torch.cuda.empty_cache()
            other = "fp16" if args.dtype == "bf16" else "bf16"
            for key, kw in ((other, dict(dtype=other)), ("full_masks", dict(full_masks=True)), ("dense_text", dict(dense_text=True)),
                            ("fp16_unguarded", dict(unguarded=True)), ("clip1", dict(clip=1.0)),
                            ("reference_dropout", dict(reference_dropout=True)), ("single_batch", dict(n_batches=1))):
                v, ms = timed_variant(pkg, args, device, **kw)
                out[f"value_{key}"], out[f"ms_per_step_{key}"] = round(v, 2), round(ms, 3)
            v5, ms5 = timed_variant(pkg, args, device, config=5)
            out["value_config5"], out["ms_per_step_config5"] = round(v5, 2), round(ms5, 3)
            out["roofline_config5"] = {"bound": "mfma", "kernel": "whole step", "achieved": round(FLOP_PER_MEME[5] * v5 / 1e12, 1),
                                       "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(FLOP_PER_MEME[5] * v5 / (MFMA_PEAK_TFLOPS * 1e12), 4),
                                       "traffic": None, "workload": "BASELINE configs[4]: CLIP ViT-L/14@336 (577 tokens) + BERT-large, seq 256, batch 32, "
                                                                    "fwd+CE+bwd+Adam, 762 M parameters; per-kernel figures: bench.py --config 5"}
            c2 = bench_config2(args)
            out["value_config2"], out["ms_per_step_config2"], out["unit_config2"] = c2["value"], c2["ms_per_step"], c2["unit"]
            out["roofline_config2"] = dict(c2["roofline"], workload=c2["config"]["workload"])
        if args.full and not args.no_cpu_baseline and world == 1:
            if args.config == 5:      # 1.6 TFLOP per meme: a batch of 32 would take the host cores an hour
                out["cpu_baseline"] = cpu_baseline(1, args.seq, args.tiny, warm=1, timed=2, config=5)
            else:
                out["cpu_baseline"] = cpu_baseline(args.cpu_batch, args.seq, args.tiny)
        print(json.dumps(out), flush=True)
    if world > 1 or args.force_ddp:
        dist.barrier()
        from multimodal_propaganda_meme_classification_amd import ddp
        ddp.shutdown()          # GraphedSteps, reducers, gc, then the process group -- in that order


if __name__ == "__main__":
    main()
