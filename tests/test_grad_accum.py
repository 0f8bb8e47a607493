"""Host side of gradient accumulation over micro-batches: the window arithmetic of the two training loops (stub model, CPU), the
switch and its clearing rule on the modules, and the declarations of the two new entry points."""
import importlib

import pytest
import torch
import torch.nn as nn

import multimodal_propaganda_meme_classification_amd as pkg
from multimodal_propaganda_meme_classification_amd import _lib

kevin = importlib.import_module("multimodal_propaganda_meme_classification_amd.kevin")
train_mod = importlib.import_module("multimodal_propaganda_meme_classification_amd.train")      # (the package exports its train() under that name)


class _Stub(nn.Module):
    """loss of a batch = w * c (c = the batch's `text` value), so d loss / d w = c: the gradient at a step tells which batches are in it."""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(()))
        self.switch = []

    def set_grad_accumulation(self, on=True):
        self.switch.append(bool(on))
        return self

    def forward(self, text, image, mask, *more):
        return (self.w * text.float().mean()).expand(text.shape[0], 2) if not more else (self.w * text.float().mean()).expand(text.shape[0])


class _Opt:
    def __init__(self, model, log):
        self.model, self.log = model, log

    def zero_grad(self):
        self.model.w.grad = None
        self.log.append("zero")

    def step(self):
        self.log.append(("step", round(float(self.model.w.grad), 6)))


class _Sched:
    def __init__(self, log):
        self.log = log

    def step(self):
        self.log.append("sched")

    def get_last_lr(self):
        return [0.0]


class _Loader(list):
    @property
    def dataset(self):
        return range(sum(b["text"].shape[0] for b in self))


def _loader(values, B=2, kevin_keys=False):
    out = _Loader()
    for c in values:
        b = {"text": torch.full((B, 3), float(c)), "image": torch.zeros((B, 3, 4, 4)), "text_mask": torch.ones((B, 3), dtype=torch.long),
             "label": torch.zeros(B, dtype=torch.long)}
        if kevin_keys:
            b.update(caption_text=torch.zeros((B, 3), dtype=torch.long), caption_text_mask=torch.ones((B, 3), dtype=torch.long))
        out.append(b)
    return out


def _mean_first_column(output, labels, **kw):
    return output.reshape(output.shape[0], -1)[:, 0].mean()


def test_train_loop_windows():
    """train.train: N = 1 is zero_grad / step per batch with the undivided loss and never touches the switch; N = 2 over five
    batches steps after batches 2, 4 and 5 (the short last window) with (c1 + c2) / 2, (c3 + c4) / 2, c5 / 2; the scheduler steps
    once per window; the reported loss is the undivided mean."""
    values = [1.0, 2.0, 4.0, 8.0, 16.0]
    model, log = _Stub(), []
    with torch.no_grad():
        model.w.fill_(1.0)
    loss, _ = train_mod.train(model, _loader(values), _mean_first_column, _Opt(model, log), "cpu")
    assert log == [x for c in values for x in ("zero", ("step", c))] and model.switch == []
    assert loss == pytest.approx(sum(values) / len(values))
    model, log = _Stub(), []
    with torch.no_grad():
        model.w.fill_(1.0)
    loss, _ = train_mod.train(model, _loader(values), _mean_first_column, _Opt(model, log), "cpu", accumulation_steps=2, scheduler=_Sched(log))
    assert log == ["zero", ("step", 1.5), "sched", "zero", ("step", 6.0), "sched", "zero", ("step", 8.0), "sched"]
    assert model.switch == [True]
    assert loss == pytest.approx(sum(values) / len(values))
    model, log = _Stub(), []
    train_mod.train(model, _loader(values[:4]), _mean_first_column, _Opt(model, log), "cpu", accumulation_steps=4)
    assert log == ["zero", ("step", 3.75)]
    with pytest.raises(ValueError, match="accumulation_steps"):
        train_mod.train(model, _loader(values), _mean_first_column, _Opt(model, log), "cpu", accumulation_steps=0)


def test_kevin_train_loop_windows():
    """kevin.train: the same windows, with the scheduler the loop always had; N = 1 is the loop as it was, call for call."""
    values = [1.0, 2.0, 4.0, 8.0, 16.0]
    pipe = lambda images: images      # noqa: E731  (the batches carry float images: the pipeline is not called)
    model, log = _Stub(), []
    kevin.train(model, _loader(values, kevin_keys=True), _mean_first_column, _Opt(model, log), _Sched(log), "cpu", 0, image_pipeline=pipe, log_every=0)
    assert log == [x for c in values for x in ("zero", ("step", c), "sched")] and model.switch == []
    model, log = _Stub(), []
    kevin.train(model, _loader(values, kevin_keys=True), _mean_first_column, _Opt(model, log), _Sched(log), "cpu", 0, image_pipeline=pipe, log_every=0,
                accumulation_steps=2)
    assert log == ["zero", ("step", 1.5), "sched", "zero", ("step", 6.0), "sched", "zero", ("step", 8.0), "sched"]
    assert model.switch == [True]
    model, log = _Stub(), []
    kevin.train(model, _loader(values, kevin_keys=True), _mean_first_column, _Opt(model, log), _Sched(log), "cpu", 0, image_pipeline=pipe, log_every=0,
                accumulation_steps=8)
    assert log == ["zero", ("step", round(sum(values) / 8, 6)), "sched"]
    with pytest.raises(ValueError, match="accumulation_steps"):
        kevin.train(model, _loader(values, kevin_keys=True), _mean_first_column, _Opt(model, log), _Sched(log), "cpu", 0, image_pipeline=pipe,
                    accumulation_steps=0)


def _tiny(**kw):
    tc = pkg.TextConfig(vocab_size=64, hidden=128, layers=1, heads=2, intermediate=128, max_position=16)
    ic = pkg.ImageConfig(image_size=16, patch=16, hidden=128, layers=1, heads=2, intermediate=128)
    return pkg.MultimodalClassifier.from_config(pkg.ModelConfig(text=tc, image=ic, proj=128, **kw))


def test_switch_and_clearing_rule_on_the_modules():
    """The switch is off by default, a runtime property (not in the config's dict form), reaches every HIP tower of a composite, and
    the three clearing routes are seen: the module's own zero_grad(), .grad is None after a parent's zero_grad(), and
    memehip.Adam.zero_grad() before the optimizer is bound."""
    m = _tiny()
    assert m.grad_accumulation is False and m._grads_cleared()
    assert m.set_grad_accumulation(True) is m and m.grad_accumulation is True
    assert "accum" not in str(m.config.to_dict()) and pkg.ModelConfig.from_dict(m.config.to_dict()).to_dict() == m.config.to_dict()
    with pytest.raises(AttributeError):
        m.grad_accumulation = False
    m._cleared = False                      # as a backward leaves it
    assert not m._grads_cleared()
    m.zero_grad()
    assert m._grads_cleared() and all(p.grad is None for p in m.parameters())
    m._attach_grads()
    m._cleared = False
    parent = pkg.TrainerModel(m)
    parent.zero_grad()                      # nn.Module.zero_grad on the parent: the child's method is not called
    assert m._cleared is False and m._grads_cleared()
    m._attach_grads()
    assert not m._grads_cleared()
    parent.zero_grad(set_to_none=False)     # zeroed in place: the next backward adds to zeros
    assert not m._grads_cleared() and float(m.flat_grads.abs().max()) == 0.0
    pkg.Adam(m.parameters(), lr=1e-3).zero_grad()
    assert m._cleared is True
    assert parent.grad_accumulation and not parent.set_grad_accumulation(False).grad_accumulation and not m.grad_accumulation
    # switching it on starts a new window
    m._cleared = False
    m.set_grad_accumulation(True)
    assert m._grads_cleared()
    # a composite with two towers and a plain-torch head
    tc = pkg.TextConfig(vocab_size=64, hidden=128, layers=1, heads=2, intermediate=128, max_position=16)
    kv = pkg.KevinMultimodalClassifier("concatenation", text=tc, image="resnet18", caption=tc, proj=128, resnet_layers=(1, 1, 1, 1))
    assert not kv.grad_accumulation
    kv.set_grad_accumulation(True)
    assert kv.grad_accumulation and kv.text_model.grad_accumulation and kv.caption_text_model.inner.grad_accumulation
    enc = pkg.TextEncoder(tc)
    assert enc.set_grad_accumulation(True) is enc and enc.grad_accumulation


def test_refusals_need_no_device():
    """forward_backward and GraphedStep refuse before they touch the device."""
    m = _tiny().set_grad_accumulation(True)
    x = torch.zeros((1, 4), dtype=torch.long)
    with pytest.raises(ValueError, match="autograd path"):
        m.forward_backward(x, torch.zeros((1, 3, 16, 16)), x, torch.zeros(1, dtype=torch.long))
    with pytest.raises(ValueError, match="reducer hooks"):
        m.forward_backward(x, torch.zeros((1, 3, 16, 16)), x, torch.zeros(1, dtype=torch.long), grad_hook=lambda *a: None)
    with pytest.raises(ValueError, match="set_grad_accumulation"):
        pkg.GraphedStep(m, pkg.Adam(m.parameters(), lr=1e-3), 1, 4)


def test_new_entry_points_are_declared():
    import ctypes as C
    assert {"mh_accum_spans_f32", "mh_bert_embed_bwd_accum"} <= set(_lib.EXPORTED_SYMBOLS)
    assert _lib._SIGNATURES["mh_bert_embed_bwd_accum"] == _lib._SIGNATURES["mh_bert_embed_bwd"]
    assert C.sizeof(_lib.MhSpanJob) == 24 and _lib.MH_SPAN_MAX_JOBS == 16
    assert _lib.MH_GEMM_ACCUM == 4          # the flag the adding weight-gradient GEMMs set: its meaning is not changed
