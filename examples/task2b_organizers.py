#!/usr/bin/env python
"""The organizers' Subtask-2B example (example_scripts/ResNet_example_task2B.py) on the MI355X path, written the way the reference writes it:

    config = ResNetConfig(num_channels=1, layer_type="basic", depths=[2, 2], hidden_sizes=[32, 64], num_labels=num_labels)
    model = ResNetForImageClassification(config)                        -> memehip.HFResNetForImageClassification(config)
    _transforms = Compose([Resize(256), CenterCrop(224), ToTensor(), Normalize(mean=[0.45], std=[0.22])])
    ... _transforms(pil_img.convert("L"))                               -> memehip.data.DeviceImagePipeline(grayscale=True, mean=(0.45,),
                                                                           std=(0.22,)): one H2D copy per batch, HIP kernels
    Trainer(model, training_args, train_dataset, data_collator=collate_fn).train() / .evaluate() / .predict()
    -> task2B_TeamName.tsv  (id <tab> label <tab> run_id)

The model has transformers' state_dict (183 554 parameters), so ``model.load_state_dict(hf_model.state_dict())`` works both ways.  The
datasets apply the transform when a batch is fetched (``__getitems__``, what ``set_transform`` does in the reference), so the whole batch goes
through the pipeline at once and arrives on the device; ``collate_fn`` is the reference's.

    python examples/task2b_organizers.py --train train.json --dev dev.json [--image-root DIR] [--synthetic-images] [--output-dir DIR]

--synthetic-images: the JSON files are read, the image files are not (absent offline): every image is noise seeded by its path.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_propaganda_meme_classification_amd as memehip

L2ID = {"not_propaganda": 0, "propaganda": 1}
ID2L = {v: k for k, v in L2ID.items()}
MODEL_NAME = "resnet50"          # the reference's run_id column (its `model_name`)


def read_data(fpath, is_test=False):
    """the reference's read_data: id, image path (and class_label) of every object of the JSON list"""
    data = {"id": [], "image": []} if is_test else {"id": [], "image": [], "label": []}
    for obj in json.load(open(fpath, encoding="utf-8")):
        data["id"].append(obj["id"])
        data["image"].append(obj["img_path"])
        if not is_test:
            data["label"].append(L2ID[obj["class_label"]])
    return data


def synthetic_image(key, size=256):
    seed = int.from_bytes(hashlib.blake2s(str(key).encode("utf-8"), digest_size=8).digest(), "little") % (2 ** 31)
    return np.random.default_rng(seed).integers(0, 256, (size, size + size // 4, 3), dtype=np.uint8)


class ImageDataset(torch.utils.data.Dataset):
    """ids, images (paths, PIL images or decoded uint8 [h, w, 3] arrays) and labels; the transform runs per fetched BATCH on the device."""

    def __init__(self, ids, images, labels, pipeline, image_root="", synthetic_images=False):
        self.ids, self.images, self.labels = list(ids), list(images), (None if labels is None else list(labels))
        self.pipeline, self.image_root, self.synthetic = pipeline, image_root, synthetic_images

    def __len__(self):
        return len(self.ids)

    def _decode(self, i):
        im = self.images[i]
        if not isinstance(im, str):
            return im
        if self.synthetic:
            return synthetic_image(im)
        from PIL import Image
        return Image.open(os.path.join(self.image_root, im))

    def __getitems__(self, indices):
        pixel_values = self.pipeline([self._decode(i) for i in indices])
        return [{"pixel_values": pixel_values[k], "label": 0 if self.labels is None else self.labels[i], "id": self.ids[i]}
                for k, i in enumerate(indices)]

    def __getitem__(self, i):
        return self.__getitems__([i])[0]


def collate_fn(examples):
    pixel_values = torch.stack([example["pixel_values"] for example in examples])
    labels = torch.tensor([example["label"] for example in examples])
    return {"pixel_values": pixel_values, "labels": labels}


def training_arguments(output_dir="./resnet_50/", **overrides):
    """the reference's TrainingArguments (its ``local_rank=1`` left out: one process; ``load_best_model_at_end`` too, which needs the
    checkpoints ``save_strategy="no"`` never writes); the batches are device tensors already, so nothing is pinned"""
    from transformers import TrainingArguments
    kw = dict(learning_rate=2e-5, num_train_epochs=2, per_device_train_batch_size=16, per_device_eval_batch_size=16, output_dir=output_dir,
              remove_unused_columns=False, save_total_limit=2, save_strategy="no", report_to=[], dataloader_pin_memory=False)
    kw.update(overrides)
    return TrainingArguments(**kw)


def compute_metrics(p):
    preds = p.predictions[0] if isinstance(p.predictions, tuple) else p.predictions
    return {"accuracy": (np.argmax(preds, axis=1) == p.label_ids).astype(np.float32).mean().item()}


def write_predictions(path, ids, predictions, run_id=MODEL_NAME):
    with open(path, "w") as writer:
        writer.write("id\tlabel\trun_id\n")
        for i, item in zip(ids, np.argmax(predictions, axis=1)):
            writer.write(f"{i}\t{ID2L[int(item)]}\t{run_id}\n")


def build_model(num_labels=2, compute_dtype="fp16"):
    from transformers import ResNetConfig
    config = ResNetConfig(num_channels=1, layer_type="basic", depths=[2, 2], hidden_sizes=[32, 64], num_labels=num_labels)
    return memehip.HFResNetForImageClassification(config, compute_dtype=compute_dtype)


def build_pipeline(image_size=224, resize=256, device="cuda"):
    return memehip.data.DeviceImagePipeline(image_size, resize, "center_crop", device=device, grayscale=True, mean=(0.45,), std=(0.22,))


def run(train, dev, output_dir, pipeline, **overrides):
    """train / evaluate / predict as the reference's cells do; `train`, `dev`: read_data dicts (images: paths, PIL images or arrays)"""
    from transformers import Trainer
    root, synth = overrides.pop("image_root", ""), overrides.pop("synthetic_images", False)
    train_ds = ImageDataset(train["id"], train["image"], train["label"], pipeline, root, synth)
    dev_ds = ImageDataset(dev["id"], dev["image"], dev["label"], pipeline, root, synth)
    model = build_model(num_labels=len(L2ID))
    trainer = Trainer(model=model, args=training_arguments(output_dir, **overrides), train_dataset=train_ds, compute_metrics=compute_metrics,
                      data_collator=collate_fn)
    train_result = trainer.train()
    metrics = trainer.evaluate(eval_dataset=dev_ds)
    predictions = trainer.predict(dev_ds, metric_key_prefix="predict").predictions
    out = os.path.join(output_dir, "task2B_TeamName.tsv")
    if trainer.is_world_process_zero():
        write_predictions(out, dev_ds.ids, predictions)
    return trainer, train_result, metrics, predictions, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", default="arabic_memes_propaganda_araieval_24_train.json")
    ap.add_argument("--dev", default="arabic_memes_propaganda_araieval_24_dev.json")
    ap.add_argument("--image-root", default="")
    ap.add_argument("--synthetic-images", action="store_true", help="do not open the image files: noise seeded by each path")
    ap.add_argument("--output-dir", default="./resnet_50/")
    args = ap.parse_args()
    os.makedirs(args.output_dir, exist_ok=True)
    _, train_result, metrics, predictions, out = run(read_data(args.train), read_data(args.dev), args.output_dir, build_pipeline(),
                                                     image_root=args.image_root, synthetic_images=args.synthetic_images)
    print({"train": train_result.metrics, "eval": metrics, "predictions": list(predictions.shape), "written": out})


if __name__ == "__main__":
    main()
