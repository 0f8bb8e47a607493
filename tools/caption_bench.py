#!/usr/bin/env python3
"""BLIP captioning throughput: blip.BlipCaptioner (hipGraph replay and eager launches) against transformers'
BlipForConditionalGeneration.generate in fp16 on the same GPU, runs alternating.

BLIP-large dimensions (ViT-L/16 at 384 px, 12-layer BERT-base decoder with 1024-wide cross-attention), random weights from --seed,
a 5-token prompt shaped like the processor's "[CLS] a meme of [SEP]", --batch images (64, the reference's batch) and
--max-new-tokens (128, the reference's).  Random weights rarely emit eos, so all steps usually run: the steps actually run are
reported next to every rate.  Prints one JSON line; --out also writes it to a file.

--repetition-penalty / --no-repeat-ngram-size / --min-length / --min-new-tokens: a further run, ours_graph_processed, with these
generate() settings joins the alternation (the other runs stay without them), and its time over the plain graph run's is reported.

--do-sample (with --temperature / --top-k / --top-p, generate()'s defaults 1.0 / 50 / 1.0): two further runs join the alternation,
ours_graph_sampled and transformers' fp16 generate(do_sample=True) with the same settings (hf_fp16_sampled); the sampled run's time
over the greedy graph run's and the sampled step's time are reported.  Greedy decoding only (--num-beams 1).

  python tools/caption_bench.py --out profiles/r05_caption_bench.json
  rocprofv3 --kernel-trace --stats -d DIR -o caption -- python tools/caption_bench.py --runs 1 --no-hf      (kernel table)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def large_config():
    from transformers import BlipConfig
    return BlipConfig(text_config=dict(encoder_hidden_size=1024, num_attention_heads=12),
                      vision_config=dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16,
                                         image_size=384, patch_size=16))


def random_state(model, seed, std=0.02):
    g = torch.Generator().manual_seed(seed)
    sd = model.state_dict()
    with torch.no_grad():
        for k, v in sd.items():
            if v.dtype.is_floating_point:
                ln = k.endswith("weight") and any(s in k for s in ("LayerNorm", "layer_norm", "layernorm"))
                v.copy_(torch.ones_like(v) if ln else std * torch.randn(v.shape, generator=g).to(v.device))
        # BLIP ties the LM head's decoder to the word embeddings and its bias to predictions.bias
        sd["text_decoder.cls.predictions.decoder.weight"].copy_(sd["text_decoder.bert.embeddings.word_embeddings.weight"])
        sd["text_decoder.cls.predictions.decoder.bias"].copy_(sd["text_decoder.cls.predictions.bias"])
    model.load_state_dict(sd)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--max-new-tokens", type=int, default=128)
    ap.add_argument("--runs", type=int, default=3, help="alternating rounds (after one warm-up round)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dtype", choices=("fp16", "bf16"), default="fp16")
    ap.add_argument("--no-hf", action="store_true", help="skip transformers' generate (e.g. under a profiler)")
    ap.add_argument("--num-beams", type=int, default=1, help="beam search with this many beams on both sides (1: greedy)")
    ap.add_argument("--repetition-penalty", type=float, default=1.0)
    ap.add_argument("--no-repeat-ngram-size", type=int, default=0)
    ap.add_argument("--min-length", type=int, default=0)
    ap.add_argument("--min-new-tokens", type=int, default=0)
    ap.add_argument("--do-sample", action="store_true", help="add sampled runs (ours and transformers') with the settings below")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=50)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    proc = dict(repetition_penalty=args.repetition_penalty, no_repeat_ngram_size=args.no_repeat_ngram_size, min_length=args.min_length,
                min_new_tokens=args.min_new_tokens)
    processed = proc != dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, min_new_tokens=0)

    samp = dict(do_sample=True, temperature=args.temperature, top_k=args.top_k, top_p=args.top_p)
    if args.do_sample and args.num_beams != 1:
        ap.error("--do-sample needs --num-beams 1")

    import __graft_entry__ as g
    g.build()
    from multimodal_propaganda_meme_classification_amd import BlipCaptioner, ops
    dev = torch.device("cuda:0")
    cfg = large_config()
    B, N, K = args.batch, args.max_new_tokens, args.num_beams
    ours = BlipCaptioner.from_config(cfg, compute_dtype=args.dtype, device=dev)
    random_state(ours, args.seed)
    hf = None
    if not args.no_hf:
        from transformers import BlipForConditionalGeneration
        with torch.device(dev):
            hf = BlipForConditionalGeneration(cfg)
        hf.load_state_dict(ours.state_dict())
        hf = hf.half().eval()
    pix = torch.randn(B, 3, 384, 384, generator=torch.Generator().manual_seed(args.seed + 1)).to(dev)
    prompt = torch.tensor([[101, 1037, 2033, 1997, 102]] * B)

    # with logits-processor settings the graph run WITH them joins the alternation; the other runs stay without (the baseline)
    runs = {"ours_graph": [], "ours_graph_processed": [], "ours_eager": [], "hf_fp16": []}
    if not processed:
        del runs["ours_graph_processed"]
    if args.do_sample:
        runs.update({"ours_graph_sampled": [], "hf_fp16_sampled": []})
    steps = {}
    for r in range(args.runs + 1):
        for name in runs:
            if name.startswith("hf_fp16") and hf is None:
                continue
            if name == "hf_fp16_sampled":
                dt, out = timed(lambda: hf.generate(pixel_values=pix.half(), input_ids=prompt.clone().to(dev), max_new_tokens=N, **samp))
            elif name == "ours_graph_sampled":
                dt, out = timed(lambda: ours.generate(pix, prompt.clone(), max_new_tokens=N, seed=args.seed + r, **samp))
            elif name == "hf_fp16":
                dt, out = timed(lambda: hf.generate(pixel_values=pix.half(), input_ids=prompt.clone().to(dev), max_new_tokens=N, num_beams=K))
            elif name == "ours_graph_processed":
                dt, out = timed(lambda: ours.generate(pix, prompt.clone(), max_new_tokens=N, num_beams=K, **proc))
            else:
                dt, out = timed(lambda: ours.generate(pix, prompt.clone(), max_new_tokens=N, graph=(name == "ours_graph"), num_beams=K))
            steps[name] = int(out.shape[1]) - (prompt.shape[1] - 1)          # new tokens in the output
            if r > 0:
                runs[name].append(dt)

    # pieces of one BlipCaptioner batch: the vision tower, the cross k / v GEMMs, one decode step (graph replay and eager)
    vis = [timed(lambda: ours.vision_forward(pix))[0] for _ in range(3)]
    st = ours._states[next(iter(ours._states))]
    n_rep = 50
    t_dev = st["sv"] if st["beam"] is None else st["beam"]["state"]

    def rewind():          # beam search: time steps inside the caption (past max_length the beam step has nothing to select)
        if st["beam"] is not None:
            t_dev[0] = prompt.shape[1] - 1
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def graph_step_ms(**kw):          # the captured step of a generate() with these settings (a call re-captures it when they differ)
        ours.generate(pix, prompt.clone(), max_new_tokens=N, num_beams=K, **kw)
        rewind()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n_rep):
            st["graph"].replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n_rep
    step_graph_processed_ms = graph_step_ms(**proc) if processed else None
    step_graph_sampled_ms = graph_step_ms(seed=args.seed, **samp) if args.do_sample else None
    step_graph_ms = graph_step_ms()
    rewind()
    e0.record()
    for _ in range(10):
        ours._step(st)
    e1.record()
    torch.cuda.synchronize()
    step_eager_ms = e0.elapsed_time(e1) / 10
    # launches per token: one per library call of the step, plus the combine launch of every split attention
    rewind()
    calls = []
    orig = ops.check
    ops.check = lambda status, what: (calls.append(what), orig(status, what))[1]
    try:
        ours._step(st)
    finally:
        ops.check = orig
    torch.cuda.synchronize()
    H = cfg.text_config.num_attention_heads
    attn = sum(1 for c in calls if c.startswith("mh_attn_decode"))
    splits = attn // 2 * ((ops.decode_splits(B * K, H, st["cap"]) > 1) + (ops.decode_splits(B * K, H, st["Ni"]) > 1))
    launches = len(calls) + splits + (1 if K > 1 else 0)          # mh_beam_step is two launches

    def stat(v):
        return {"median_s": sorted(v)[len(v) // 2], "runs_s": [round(x, 4) for x in v]} if v else None

    res = {"metric": f"BLIP-large captioning images/s ({'greedy' if K == 1 else f'beam search, {K} beams'}, fp16 reference)", "batch": B, "max_new_tokens": N, "dtype": args.dtype,
           "weights": f"random, seed {args.seed}", "gpu": torch.cuda.get_device_name(0)}
    for name, v in runs.items():
        if v:
            res[name] = dict(stat(v), images_per_s=round(B / stat(v)["median_s"], 2), new_tokens=steps[name],
                             ms_per_new_token=round(1000 * stat(v)["median_s"] / max(1, steps[name]), 3))
    res["vision_tower_ms"] = round(1000 * sorted(vis)[1], 3)
    res["decode_step_ms_graph"] = round(step_graph_ms, 4)
    res["decode_step_ms_eager"] = round(step_eager_ms, 4)
    if processed:
        res["logits_processors"] = proc
        res["decode_step_ms_graph_processed"] = round(step_graph_processed_ms, 4)
        res["processed_over_plain_time"] = round(stat(runs["ours_graph_processed"])["median_s"] / stat(runs["ours_graph"])["median_s"], 4)
    if args.do_sample:
        res["sampling"] = {k: v for k, v in samp.items() if k != "do_sample"}
        res["decode_step_ms_graph_sampled"] = round(step_graph_sampled_ms, 4)
        res["sampled_over_greedy_time"] = round(stat(runs["ours_graph_sampled"])["median_s"] / stat(runs["ours_graph"])["median_s"], 4)
    res["launches_per_token"] = launches
    res["decode_steps_per_batch"] = prompt.shape[1] - 2 + steps["ours_graph"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
