"""train / test / evaluate with the reference's signatures (example_scripts/Multimodal_example_task2C.txt:200-282).

The loops are the reference's in behaviour: zero_grad -> forward -> criterion -> backward -> step,
running loss weighted by batch size, accuracy from argmax, both divided by ``len(loader.dataset)``;
``evaluate`` writes the 3-column TSV ``id<TAB>label<TAB>run_id`` with the header the reference
writes (:275), which the task's format checker and scorer accept.
The only addition: loss / accuracy are accumulated on the GPU and read back once per epoch instead
of two ``.item()`` syncs per step (:218-220), unless ``sync_every_step=True``.
"""
from __future__ import annotations

from typing import Tuple

import torch

from .data import id2l, normalize_images


def train(model, train_loader, criterion, optimizer, device, sync_every_step: bool = False, accumulation_steps: int = 1,
          scheduler=None) -> Tuple[float, float]:
    """``accumulation_steps`` = N > 1: gradient accumulation over windows of N batches -- ``zero_grad()`` in front of a window, every
    batch's loss divided by N, ``optimizer.step()`` (and ``scheduler.step()``, when one is given) once behind it; the last window
    of an epoch may be short and steps with what it has.  The model's ``set_grad_accumulation(True)`` is called.  N = 1 is the
    reference's loop, call for call (a scheduler, which the reference's loop does not have, steps after every batch)."""
    N = int(accumulation_steps)
    if N < 1:
        raise ValueError(f"accumulation_steps must be >= 1, got {accumulation_steps}")
    model.train()
    if N > 1 and hasattr(model, "set_grad_accumulation"):       # (a plain torch module accumulates into .grad by itself)
        model.set_grad_accumulation(True)
    loss_sum = torch.zeros((), device=device)
    correct = torch.zeros((), device=device, dtype=torch.long)
    pending = 0          # backwards since the last optimizer step
    for data in train_loader:
        if pending == 0:
            optimizer.zero_grad()
        text = data["text"].to(device)
        image = normalize_images(data["image"].to(device, non_blocking=True))
        mask = data["text_mask"].to(device)
        labels = data["label"].to(device)
        output = model(text, image, mask)
        loss = criterion(output, labels)
        (loss if N == 1 else loss / N).backward()
        pending += 1
        if pending == N:
            pending = _window_step(optimizer, scheduler)
        loss_sum += loss.detach() * labels.size(0)
        _, predicted = torch.max(output.detach(), 1)
        correct += (predicted == labels).sum()
        if sync_every_step:
            loss_sum.item()
    if pending:          # the epoch's last, short window
        _window_step(optimizer, scheduler)
    n = len(train_loader.dataset)
    return float(loss_sum) / n, int(correct) / n


def _window_step(optimizer, scheduler) -> int:
    optimizer.step()
    if scheduler is not None:
        scheduler.step()
    return 0


def test(model, test_loader, criterion, device) -> Tuple[float, float]:
    model.eval()
    loss_sum = torch.zeros((), device=device)
    correct = torch.zeros((), device=device, dtype=torch.long)
    with torch.no_grad():
        for data in test_loader:
            text = data["text"].to(device)
            image = normalize_images(data["image"].to(device, non_blocking=True))
            mask = data["text_mask"].to(device)
            labels = data["label"].to(device)
            output = model(text, image, mask)
            loss = criterion(output, labels)
            loss_sum += loss * labels.size(0)
            _, predicted = torch.max(output, 1)
            correct += (predicted == labels).sum()
    n = len(test_loader.dataset)
    return float(loss_sum) / n, int(correct) / n


def evaluate(model, test_loader, device, out_path: str = "task2C_TeamName.tsv", run_id: str = "ViT-BERT-memehip") -> str:
    model.eval()
    predictions, ids = [], []
    with torch.no_grad():
        for data in test_loader:
            text = data["text"].to(device)
            image = normalize_images(data["image"].to(device, non_blocking=True))
            mask = data["text_mask"].to(device)
            output = model(text, image, mask)
            _, predicted = torch.max(output, 1)
            predictions.append(predicted.cpu())
            ids.append(data["id"])
    with open(out_path, "w") as f:
        f.write("id\tlabel\trun_id\n")
        for i, line in enumerate(predictions):
            for indx, l in enumerate(line.tolist()):
                f.write(f"{ids[i][indx]}\t{id2l[l]}\t{run_id}\n")
    return out_path
