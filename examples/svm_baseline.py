#!/usr/bin/env python
"""The organizers' "ResNet+BERT SVM" baseline of Subtask 2C (baselines/extract_feat.py + baselines/subtask_2c.py) end to end on the
MI355X path, written the way the reference writes it:

    img_feats, text_feats = get_features(loader, model, device)         -> memehip.get_features   (the HIP towers, forward only)
    json.dump({"imgfeats": ..., "textfeats": ...}, features/<split>_feats.json)  -> memehip.dump_features
    run_imgbert_baseline(data_dir, split, train_fpath, test_fpath, out) -> memehip.run_imgbert_baseline
        clf = SVC(C=1, kernel='linear', random_state=0); clf.fit(...); clf.predict(...)   -> memehip.SVC (csrc/svm.hip)
    acc, precision, recall, f1 = scorer.task2.evaluate(gold, out)       -> the same four numbers, printed as the scorer prints them

A synthetic split (no dataset offline): texts whose vocabulary leans with the label, pseudo-images per id, a small two-tower model
with random weights.   python examples/svm_baseline.py [--train 96] [--dev 48] [--image-only]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_propaganda_meme_classification_amd as memehip

LABELS = ("not_propaganda", "propaganda")


def synthetic_split(n, seed):
    rng = np.random.default_rng(seed)
    words = [f"w{i}" for i in range(200)]
    out = []
    for k in range(n):
        lab = int(rng.random() < 0.28)
        lean = np.r_[np.full(100, 3.0 if lab else 1.0), np.full(100, 1.0 if lab else 3.0)]
        text = " ".join(rng.choice(words, size=12, p=lean / lean.sum()))
        out.append({"id": f"data/synthetic/images/s{seed}_{k:04d}.jpg", "img_path": f"s{seed}_{k:04d}.jpg", "text": text,
                    "class_label": LABELS[lab]})
    return out


def scores(gold, pred):
    """accuracy, weighted precision, weighted recall, macro F1: scorer/task2.py's four sklearn.metrics calls"""
    gold, pred = np.asarray(gold), np.asarray(pred)
    p, r, f, w = [], [], [], []
    for lab in sorted(set(gold) | set(pred)):
        tp = float(((pred == lab) & (gold == lab)).sum())
        pp, gp = float((pred == lab).sum()), float((gold == lab).sum())
        p.append(tp / pp if pp else 0.0)
        r.append(tp / gp if gp else 0.0)
        f.append(2 * tp / (pp + gp) if pp + gp else 0.0)
        w.append(gp)
    w = np.array(w) / sum(w)
    return float((gold == pred).mean()), float(w @ p), float(w @ r), float(np.mean(f))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", type=int, default=96)
    ap.add_argument("--dev", type=int, default=48)
    ap.add_argument("--image-only", action="store_true", help="the Subtask-2B variant: run_image_baseline over imgfeats alone")
    args = ap.parse_args()
    device = torch.device("cuda")
    cfg = memehip.ModelConfig(text=memehip.TextConfig(vocab_size=512, hidden=128, layers=2, heads=2, intermediate=256, max_position=64),
                              image=memehip.ImageConfig(image_size=32, hidden=128, layers=2, heads=2, intermediate=256), proj=128)
    model = memehip.MultimodalClassifier.from_config(cfg, seed=4).to(device)
    with tempfile.TemporaryDirectory() as data_dir:
        for split, n, seed in (("train", args.train, 1), ("dev", args.dev, 2)):
            entries = synthetic_split(n, seed)
            with open(os.path.join(data_dir, f"{split}.json"), "w") as f:
                json.dump(entries, f)
            df = memehip.read_data(os.path.join(data_dir, f"{split}.json"))
            ds = memehip.MultimodalDataset(df["id"], df["text"], df["image"], [memehip.l2id[v] for v in df["label"]], max_seq_len=32,
                                           image_size=32, synthetic_images=True, vocab_size=512)
            img_feats, text_feats = memehip.get_features(torch.utils.data.DataLoader(ds, batch_size=16), model, device)
            memehip.dump_features(os.path.join(data_dir, "features", f"{split}_feats.json"), img_feats, text_feats)
        out = os.path.join(data_dir, "baseline_dev.tsv")
        run = memehip.run_image_baseline if args.image_only else memehip.run_imgbert_baseline
        clf = run(data_dir, "dev", "train.json", "dev.json", out)
        gold = {e["id"]: e["class_label"] for e in json.load(open(os.path.join(data_dir, "dev.json")))}
        rows = [ln.rstrip("\n").split("\t") for ln in open(out)][1:]
        acc, precision, recall, f1 = scores([gold[r[0]] for r in rows], [r[1] for r in rows])
    print(f"SVC on the device: {int(clf.n_iter_[0])} iterations, {int(clf.n_support_.sum())} support vectors of {args.train}, "
          f"fit_status {clf.fit_status_}")
    print("acc: {}, P:{}, R:{}, F1:{}".format(acc, precision, recall, f1))


if __name__ == "__main__":
    main()
