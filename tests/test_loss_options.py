"""Host side of the loss options: constructor validation, the class weights stay out of every state_dict, sklearn's 'balanced'
rule, and the C entries' declarations.  (The kernels: tests/test_loss_options_gpu.py.)"""
import numpy as np
import pytest
import torch

import multimodal_propaganda_meme_classification_amd as pkg


def test_cross_entropy_constructor_validation():
    crit = pkg.CrossEntropyLoss()
    assert crit.weight is None and crit.ignore_index is None and crit.label_smoothing == 0.0 and crit.reduction == "mean"
    assert crit._plain
    crit = pkg.CrossEntropyLoss(weight=np.array([0.5, 2.0]), ignore_index=-100, label_smoothing=0.1, reduction="none")
    assert crit.weight.dtype == torch.float32 and crit.weight.tolist() == [0.5, 2.0] and not crit._plain
    for kw in (dict(reduction="batchmean"), dict(label_smoothing=-0.1), dict(label_smoothing=1.5), dict(label_smoothing=float("nan")),
               dict(label_smoothing="0.1"), dict(ignore_index=1.5), dict(ignore_index=True), dict(weight=[[1.0, 2.0]]), dict(weight=[]),
               dict(weight=[1.0, -1.0]), dict(weight=[1.0, float("inf")]), dict(weight=[1.0, float("nan")])):
        with pytest.raises(ValueError):
            pkg.CrossEntropyLoss(**kw)
    for kw in (dict(ignore_index=0), dict(label_smoothing=1e-3), dict(reduction="sum"), dict(weight=[1.0, 1.0])):
        assert not pkg.CrossEntropyLoss(**kw)._plain, kw


def test_bce_constructor_validation():
    assert pkg.BCEWithLogitsLoss().pos_weight == 1.0
    assert pkg.BCEWithLogitsLoss(pos_weight=torch.tensor([2.5])).pos_weight == 2.5
    for kw in (dict(reduction="none"), dict(pos_weight=-1.0), dict(pos_weight=float("nan")), dict(pos_weight=torch.ones(2))):
        with pytest.raises(ValueError):
            pkg.BCEWithLogitsLoss(**kw)
    with pytest.raises(pkg.MemehipError):           # no CPU fallback
        pkg.BCEWithLogitsLoss()(torch.zeros(3, 1), torch.zeros(3))


def test_set_loss_options_validation_and_key():
    from multimodal_propaganda_meme_classification_amd.engine import LossOptions
    model = pkg.MultimodalClassifier.from_config(_tiny(), init=False)
    assert model.loss_options is None
    model.set_loss_options(weight=[1.0, 3.0], ignore_index=-100, label_smoothing=0.25, reduction="sum")
    assert model.loss_options == LossOptions(True, -100, 0.25, "sum") and hash(model.loss_options) is not None
    buf = model._loss_weight
    model.set_loss_options(weight=[2.0, 5.0])
    assert model._loss_weight is buf and buf.tolist() == [2.0, 5.0], "new values go into the one buffer"
    assert model.loss_options == LossOptions(True, None, 0.0, "mean")
    model.set_loss_options()
    assert model.loss_options is None and model._loss_weight is buf
    assert not [k for k in model.state_dict() if "loss" in k]
    for kw in (dict(reduction="none"), dict(weight=[1.0]), dict(label_smoothing=2.0), dict(ignore_index="x")):
        with pytest.raises(ValueError):
            model.set_loss_options(**kw)


def _tiny():
    return pkg.ModelConfig(text=pkg.TextConfig(vocab_size=64, hidden=128, layers=1, heads=2, intermediate=256, max_position=16),
                           image=pkg.ImageConfig(image_size=32, patch=16, hidden=128, layers=1, heads=2, intermediate=256),
                           proj=128, num_classes=2)


def _models():
    text = pkg.TextConfig(vocab_size=64, hidden=128, layers=1, heads=2, intermediate=256, max_position=16)
    yield "HFResNetForImageClassification", lambda: pkg.HFResNetForImageClassification(
        embedding_size=8, hidden_sizes=[8, 16], depths=[1, 1], layer_type="basic", num_labels=2)
    yield "TextClassifier", lambda: pkg.TextClassifier(text, pooling_type="cls", num_classes=2)
    yield "TrainerModel", lambda: pkg.TrainerModel(pkg.MultimodalClassifier.from_config(_tiny()))
    yield "ResNetClassifier", lambda: pkg.ResNetClassifier(num_labels=2, arch="resnet18", layers=(1, 1, 1, 1))


@pytest.mark.parametrize("name,make", list(_models()), ids=[n for n, _ in _models()])
def test_state_dict_is_unchanged_by_a_weighted_loss_fct(name, make):
    """The class weights are a non-persistent buffer: state_dict() keeps its keys, key for key and in order, and a strict load of a
    checkpoint written without them still passes."""
    model = make()
    keys = list(model.state_dict().keys())
    assert keys and not [k for k in keys if k.startswith("loss_fct")]
    model.loss_fct = pkg.CrossEntropyLoss(weight=pkg.balanced_class_weights([0, 0, 0, 1]), label_smoothing=0.1, ignore_index=-100)
    assert list(model.state_dict().keys()) == keys
    assert [n for n, _ in model.named_buffers() if n == "loss_fct.weight"] == ["loss_fct.weight"]
    fresh = make()
    fresh.loss_fct = pkg.CrossEntropyLoss(weight=[1.0, 2.0])
    fresh.load_state_dict(model.state_dict(), strict=True)
    make().load_state_dict(fresh.state_dict(), strict=True)


def test_balanced_class_weights_closed_form():
    w = pkg.balanced_class_weights(torch.tensor([0] * 1500 + [1] * 643))
    assert w.dtype == np.float64 and np.array_equal(w, 2143 / (2 * np.array([1500.0, 643.0])))
    assert np.array_equal(pkg.balanced_class_weights([1, 0]), np.array([1.0, 1.0]))
    assert np.array_equal(pkg.balanced_class_weights(np.array([0, 2, 2, 1]), num_classes=3), 4 / (3 * np.array([1.0, 1.0, 2.0])))
    for bad in ([], [0, 2], [-1, 0], [0.5, 1.0]):
        with pytest.raises(ValueError):
            pkg.balanced_class_weights(bad)
    with pytest.raises(ValueError):
        pkg.balanced_class_weights([0, 1, 2], num_classes=2)


@pytest.mark.parametrize("counts", [(1, 1), (3, 1), (1500, 643), (7, 2, 30)], ids=lambda c: "x".join(map(str, c)))
def test_balanced_class_weights_is_sklearns_rule(counts):
    cw = pytest.importorskip("sklearn.utils.class_weight")
    y = np.concatenate([np.full(n, c) for c, n in enumerate(counts)])
    np.random.default_rng(0).shuffle(y)
    want = cw.compute_class_weight("balanced", classes=np.arange(len(counts)), y=y)
    got = pkg.balanced_class_weights(y)
    assert got.dtype == want.dtype == np.float64 and np.array_equal(got, want)
    assert np.array_equal(pkg.balanced_class_weights(torch.from_numpy(y), num_classes=len(counts)), want)


def test_header_declares_the_loss_entries():
    """(tests/test_abi.py holds every declaration against the library's exports; this only pins the two signatures' shape.)"""
    import ctypes as C
    sig = pkg._lib._SIGNATURES
    assert sig["mh_ce_opts_fwd_bwd"][1][8:12] == [C.c_int64, C.c_int, C.c_float, C.c_int] and len(sig["mh_ce_opts_fwd_bwd"][1]) == 15
    assert sig["mh_bce_fwd_bwd"][1][3] == C.c_float and len(sig["mh_bce_fwd_bwd"][1]) == 12
    assert (pkg._lib.MH_LOSS_MEAN, pkg._lib.MH_LOSS_SUM, pkg._lib.MH_LOSS_NONE) == (0, 1, 2)
