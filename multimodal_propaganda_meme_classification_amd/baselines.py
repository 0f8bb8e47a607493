"""The organizers' feature-SVM baselines on the device: ``features.dump_features`` -> ``SVC`` -> the submission TSV.

``run_imgbert_baseline`` has the signature, the file layout and the TSV of baselines/subtask_2c.py:74-95 (the published
"ResNet+BERT SVM" row of Subtask 2C): it reads ``<data_dir>/features/train_feats.json`` and ``<data_dir>/features/<split>_feats.json``
(the ``{"imgfeats", "textfeats"}`` files ``features.dump_features`` writes), concatenates image + text features per id and fits
``SVC(C=1, kernel='linear', random_state=0)``.  ``run_image_baseline`` is the Subtask-2B variant over the image features alone
(baselines/subtask_2b.py:76-105).  The n-gram TF-IDF baseline of 2A / 2C needs no code here: ``SVC`` takes the dense TF-IDF matrix.
"""
from __future__ import annotations

import json
from os.path import join

import numpy as np

from .svm import SVC


def _run(data_dir, split, train_fpath, test_fpath, results_fpath, parts, run_id):
    def load(*path):
        with open(join(data_dir, *path)) as f:
            return json.load(f)

    def matrix(feats, entries):
        return np.array([[v for part in parts for v in feats[part][str(e["id"])]] for e in entries], dtype=np.float64)

    train, test = load(train_fpath), load(test_fpath)
    clf = SVC(C=1, kernel="linear", random_state=0)
    clf.fit(matrix(load("features", "train_feats.json"), train), [e["class_label"] for e in train])
    labels = clf.predict(matrix(load("features", f"{split}_feats.json"), test))
    with open(results_fpath, "w") as out:
        out.write("id\tclass_label\trun_id\n")
        for e, label in zip(test, labels):
            out.write(f"{e['id']}\t{label}\t{run_id}\n")
    return clf


def run_imgbert_baseline(data_dir, split, train_fpath, test_fpath, results_fpath):
    """image + text features, run_id ``imgbert``; returns the fitted SVC (the reference returns nothing)"""
    return _run(data_dir, split, train_fpath, test_fpath, results_fpath, ("imgfeats", "textfeats"), "imgbert")


def run_image_baseline(data_dir, split, train_fpath, test_fpath, results_fpath):
    """image features alone (Subtask 2B), run_id ``image``"""
    return _run(data_dir, split, train_fpath, test_fpath, results_fpath, ("imgfeats",), "image")
