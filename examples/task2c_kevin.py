#!/usr/bin/env python
"""Kevin's three-tower Subtask-2C step (example_scripts/Multimodal_example_task2C.py:587-776) on the MI355X path, written
the way the reference writes it:

    model = MultimodalClassifier("concatenation")                       -> memehip.KevinMultimodalClassifier
    criterion = sigmoid_focal_loss                                      -> memehip.SigmoidFocalLoss
    optimizer = optim.Adam(model.get_params(lr), lr=lr)                 -> memehip.Adam (ONE optimizer, three groups, three
                                                                           flat buffers, ONE global clip norm)
    scheduler = get_linear_schedule_with_warmup(...)                    -> memehip.get_linear_schedule_with_warmup
    output = model(text, image, mask, caption_text, caption_text_mask); loss = criterion(output, labels, alpha=0.25,
    gamma=2.0, reduction="mean"); loss.backward(); clip to 1.0; optimizer.step(); scheduler.step()

Towers, poolings, Linear+BatchNorm1d+ReLU projections, ConcatAttention3, the focal loss and Adam all run in libmemehip.
Synthetic inputs (no dataset or checkpoints offline).   python examples/task2c_kevin.py [--full] [--caption-model {bert,roberta}]
                                                                                          [--image-model {vit,resnet18,convnext_tiny}]
                                                                                          [--accumulation-steps N]
                                                                                          [--criterion {focal,bce}] [--pos-weight W]
--criterion bce: ``nn.BCEWithLogitsLoss(pos_weight=...)`` in place of the focal loss -> memehip.BCEWithLogitsLoss (mh_bce_fwd_bwd);
--pos-weight is a number or ``balanced`` = n_neg / n_pos of the training labels (the class-weighted criterion the reference names
as the focal loss's alternative, :136-139, :166).
--accumulation-steps N: gradient accumulation -- every step runs the batch as N micro-batches with loss / N and one
optimizer.step() behind them (model.set_grad_accumulation(True)).
--image-model resnet18: the image tower is the submitted model's ``image_model = "resnet18"`` (:82 default; the only family its
hard-coded ``Linear(512, 512)`` admits) -- resnet.ResNet18 under FineTuneMLP(512, proj), the text tower a TextEncoder of its own.
--image-model convnext_tiny: the organizers' own image backbone (baselines/extract_feat.py) under the same head --
convnext.ConvNeXtTiny through its differentiable tower() under FineTuneMLP(768, proj); bf16, since a from-scratch layer_scale of 1e-6
underflows in fp16's folded weight (a released checkpoint's 0.1 ... 1 does not).
--caption-model roberta: the caption tower is the submitted model's ``english_text_model = "roberta-base"`` (:81) --
TextConfig.roberta_base (position ids from the input ids) with the RoBERTa tokenizers' special ids.
--caption-repetition-penalty P / --caption-no-repeat-ngram-size N / --caption-min-new-tokens M: generate() settings of the caption
stage (BlipCaptioner.generate; kevin.blip_caption_fn passes the same keywords through).  The defaults are neutral: the reference's
caption stage.  With any of them set, a small random BLIP captions the synthetic images with them and the caption tower reads
those ids.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_propaganda_meme_classification_amd as memehip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--caption-model", choices=("bert", "roberta"), default="bert")
    ap.add_argument("--image-model", choices=("vit", "resnet18", "convnext_tiny"), default="vit")
    ap.add_argument("--accumulation-steps", type=int, default=1,
                    help="N > 1: every step accumulates the gradients of N micro-batches (the batch in N parts, loss / N)")
    ap.add_argument("--criterion", choices=("focal", "bce"), default="focal")
    ap.add_argument("--pos-weight", default="1", help="with --criterion bce: a number, or 'balanced' = n_neg / n_pos of the training labels")
    ap.add_argument("--caption-repetition-penalty", type=float, default=1.0)
    ap.add_argument("--caption-no-repeat-ngram-size", type=int, default=0)
    ap.add_argument("--caption-min-new-tokens", type=int, default=0)
    args = ap.parse_args()
    small, roberta, resnet = not args.full, args.caption_model == "roberta", args.image_model == "resnet18"
    convnext = args.image_model == "convnext_tiny"
    named = args.image_model if (resnet or convnext) else None          # a tower picked by name instead of an ImageConfig
    dtype = "bf16" if convnext else "fp16"
    device = torch.device("cuda")
    torch.manual_seed(0)
    if small:
        tc = memehip.TextConfig(vocab_size=2000, hidden=128, layers=2, heads=2, intermediate=256, max_position=64)
        ic = memehip.ImageConfig(image_size=64, hidden=128, layers=2, heads=2, intermediate=256)
        cc = memehip.TextConfig(vocab_size=2000, hidden=128, layers=2, heads=2, intermediate=256, max_position=64)
        if roberta:
            cc = memehip.TextConfig.roberta_base(vocab_size=2000, hidden=128, layers=2, heads=2, intermediate=256, max_position=66)
        model = memehip.KevinMultimodalClassifier("concatenation", text=tc, image=named or ic, caption=cc, proj=128,
                                                  compute_dtype=dtype, resnet_layers=(1, 1, 1, 1) if resnet else None,
                                                  convnext_depths=(1, 1, 1, 1) if convnext else None)
        B, S = 8, 32
    else:          # AraBERT-base + ViT-B/16 + bert-base-uncased captions
        cc = memehip.TextConfig.roberta_base(hidden_dropout=0.1, attention_dropout=0.1) if roberta else None
        tc, ic = memehip.TextConfig(hidden_dropout=0.1, attention_dropout=0.1), memehip.ImageConfig()
        model = memehip.KevinMultimodalClassifier("concatenation", text=tc, image=named or ic, caption=cc, compute_dtype=dtype)
        cc = cc or memehip.TextConfig(vocab_size=30522)
        B, S = 32, 128
    model.to(device).train()
    g = torch.Generator().manual_seed(1)
    text = torch.randint(5, tc.vocab_size, (B, S), generator=g)
    cap = torch.randint(5, cc.vocab_size, (B, S), generator=g)
    lens = torch.randint(4, S + 1, (B,), generator=g)
    mask = (torch.arange(S)[None] < lens[:, None]).long()
    image = torch.randn((B, 3, ic.image_size, ic.image_size), generator=g)
    labels = (torch.rand(B, generator=g) < 0.28).float().to(device)
    caption_kw = dict(repetition_penalty=args.caption_repetition_penalty, no_repeat_ngram_size=args.caption_no_repeat_ngram_size,
                      min_new_tokens=args.caption_min_new_tokens)
    if caption_kw != dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0):
        # the caption stage (ImageCaptioning, :195-256) with these generate() settings: a random BLIP of the small towers' size writes
        # the caption ids the caption tower reads (no checkpoint or tokenizer offline, so the ids stand for themselves)
        if not small:
            ap.error("the --caption-* generate settings run the synthetic caption stage of the small configuration (omit --full)")
        blip = memehip.BlipCaptioner.from_config(dict(
            text_config=dict(vocab_size=cc.vocab_size, hidden_size=128, encoder_hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                             num_attention_heads=2, max_position_embeddings=64, bos_token_id=cc.vocab_size - 2, sep_token_id=102,
                             pad_token_id=0),
            vision_config=dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                               image_size=ic.image_size, patch_size=16)), device=device)
        for p in blip.parameters():
            torch.nn.init.normal_(p, std=0.1)
        ids = blip.generate(image.to(device), torch.tensor([[101, 7, 8, 9, 102]] * B), max_new_tokens=S - 8, **caption_kw).cpu()
        ids = ids[:, 4:]                                   # the generated part
        cap[:, :ids.shape[1]] = ids.clamp(min=5)
        print(f"caption stage: generate({caption_kw}) wrote {ids.shape[1]} tokens per image; first row {ids[0, :12].tolist()}")
    cap, cap_mask = cap * mask, mask
    if roberta:         # captions through the tokenizer: <s> words </s> <pad>...; the position ids follow the pad pattern
        tok = memehip.HashTokenizer.roberta(cc.vocab_size)
        enc = [tok.encode_plus(" ".join(f"w{int(t)}" for t in row[:n - 2]), max_length=S) for row, n in zip(cap, lens.clamp(min=2))]
        cap, cap_mask = torch.cat([e["input_ids"] for e in enc]), torch.cat([e["attention_mask"] for e in enc])
    batch = [x.to(device) for x in (text * mask, image, mask, cap, cap_mask)]

    lr = 2e-5
    optimizer = memehip.Adam(model.get_params(lr), lr=lr, max_grad_norm=1.0)      # clip_grad_norm_(model.parameters(), 1.0), fused
    scheduler = memehip.get_linear_schedule_with_warmup(optimizer, num_warmup_steps=2, num_training_steps=10)
    if args.criterion == "bce":
        n_pos = float(labels.sum())
        if args.pos_weight == "balanced":
            if n_pos == 0:
                ap.error("--pos-weight balanced: the training labels hold no positive sample")
            pos_weight = (B - n_pos) / n_pos
        else:
            try:
                pos_weight = float(args.pos_weight)
            except ValueError:
                ap.error(f"--pos-weight must be a number or 'balanced', got {args.pos_weight!r}")
        criterion = memehip.BCEWithLogitsLoss(pos_weight=pos_weight)
        print(f"criterion: BCEWithLogitsLoss(pos_weight={pos_weight:.4f})")
    else:
        criterion = memehip.SigmoidFocalLoss()
    N = args.accumulation_steps
    if N < 1 or B % N:
        ap.error(f"--accumulation-steps must divide the batch of {B}")
    if N > 1:       # the HIP towers then add every backward after the first of a window into .grad, as the rest of the model does
        model.set_grad_accumulation(True)
    for step in range(5):
        optimizer.zero_grad()
        if N == 1:
            output = model(*batch)
            loss = criterion(output, labels, alpha=0.25, gamma=2.0, reduction="mean")
            loss.backward()
        else:
            losses = []
            for k in range(N):
                part = slice(k * (B // N), (k + 1) * (B // N))
                output = model(*(x[part] for x in batch))
                micro = criterion(output, labels[part], alpha=0.25, gamma=2.0, reduction="mean")
                (micro / N).backward()
                losses.append(micro.detach())
            loss = torch.stack(losses).mean()
        grad_norm = optimizer.grad_norm()          # clip_grad_norm_(model.parameters(), float("inf")) of the reference's log line
        optimizer.step()
        scheduler.step()
        print(f"step {step}: {args.criterion} loss {float(loss.detach()):.5f} | LR {scheduler.get_last_lr()[0]:.2e} | Grad Norm {float(grad_norm):.4f}",
              flush=True)
    print("ok")


if __name__ == "__main__":
    main()
