"""RoBERTa-family text towers, host side: the configuration field and factories, the sequence-length check, the tokenizer's
special ids, and the golden fixture (tests/golden/roberta_tiny.npz, tools/gen_roberta_golden.py) against the rule as stated
in include/memehip.h.  No GPU."""
import os

import numpy as np
import pytest

from multimodal_propaganda_meme_classification_amd.config import (ImageConfig, Layout, ModelConfig, TextConfig,
                                                                  check_sequence_length)
from multimodal_propaganda_meme_classification_amd.data import HashTokenizer


def _tiny_image():
    return ImageConfig(image_size=16, patch=16, hidden=128, layers=1, heads=2, intermediate=128)


def _rule(ids, pad):
    """pad + (non-pad ids up to and including the token) for a non-pad token, pad for a pad token"""
    live = (ids != pad).astype(np.int64)
    return (np.cumsum(live, axis=1) * live + pad).astype(np.int64)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "roberta_tiny.npz"))


def test_factories():
    r = TextConfig.roberta_base()
    assert (r.vocab_size, r.max_position, r.type_vocab, r.pad_token_id, r.ln_eps, r.position_scheme) == \
        (50265, 514, 1, 1, 1e-5, "roberta")
    assert (r.hidden, r.layers, r.heads, r.intermediate) == (768, 12, 12, 3072)
    assert r.hidden_dropout == 0.0 and r.attention_dropout == 0.0
    x = TextConfig.xlm_roberta_base()
    assert x.vocab_size == 250002
    assert {k: v for k, v in vars(x).items() if k != "vocab_size"} == {k: v for k, v in vars(r).items() if k != "vocab_size"}
    o = TextConfig.roberta_base(hidden_dropout=0.1, layers=2)
    assert o.hidden_dropout == 0.1 and o.layers == 2 and o.position_scheme == "roberta"
    assert TextConfig.xlm_roberta_base(vocab_size=1000).vocab_size == 1000
    assert TextConfig().position_scheme == "absolute"


def test_validate_rejects_unknown_scheme():
    cfg = ModelConfig(text=TextConfig(position_scheme="learned"))
    with pytest.raises(ValueError, match="position_scheme"):
        cfg.validate()
    ModelConfig(text=TextConfig.roberta_base()).validate()
    ModelConfig().validate()


def test_dict_round_trip():
    cfg = ModelConfig(text=TextConfig.roberta_base(layers=2), image=_tiny_image())
    d = cfg.to_dict()
    assert d["text"]["position_scheme"] == "roberta"
    back = ModelConfig.from_dict(d)
    assert back.text == cfg.text and back.to_dict() == d
    # a dict written before the field existed still loads, as the absolute scheme
    del d["text"]["position_scheme"]
    assert ModelConfig.from_dict(d).text.position_scheme == "absolute"


def test_layout_position_table():
    lay = Layout(ModelConfig(text=TextConfig.roberta_base(layers=1), image=_tiny_image()))
    assert lay.spec["bert.embeddings.position_embeddings.weight"].shape == (514, 768)
    assert lay.spec["bert.embeddings.token_type_embeddings.weight"].shape == (1, 768)
    assert lay.spec["bert.embeddings.word_embeddings.weight"].shape == (50265, 768)


def test_sequence_length_check():
    r = TextConfig.roberta_base()
    check_sequence_length(r, 512)
    with pytest.raises(ValueError) as e:
        check_sequence_length(r, 513)
    assert all(n in str(e.value) for n in ("513", "514")) and "pad_token_id 1" in str(e.value)
    a = TextConfig()                 # absolute: S <= max_position, as before
    check_sequence_length(a, 512)
    with pytest.raises(ValueError, match="sequence length 513 > max_position 512"):
        check_sequence_length(a, 513)


def test_hash_tokenizer():
    d = HashTokenizer(1000)
    assert (d.cls_token_id, d.sep_token_id, d.pad_token_id) == (2, 3, 0) == \
        (HashTokenizer.cls_token_id, HashTokenizer.sep_token_id, HashTokenizer.pad_token_id)
    e = d.encode_plus("a b c", max_length=8)
    ids, mask = e["input_ids"][0].tolist(), e["attention_mask"][0].tolist()
    assert ids[0] == 2 and ids[4] == 3 and ids[5:] == [0, 0, 0] and mask == [1] * 5 + [0] * 3
    r = HashTokenizer.roberta(1000)
    assert (r.cls_token_id, r.sep_token_id, r.pad_token_id, r.vocab_size) == (0, 2, 1, 1000)
    f = r.encode_plus("a b c", max_length=8)
    rids = f["input_ids"][0].tolist()
    assert rids[0] == 0 and rids[4] == 2 and rids[5:] == [1, 1, 1] and f["attention_mask"][0].tolist() == mask
    assert rids[1:4] == ids[1:4] and all(t >= 5 for t in rids[1:4])       # the words hash as before, clear of the special ids
    k = HashTokenizer(1000, cls_token_id=7, sep_token_id=8, pad_token_id=9)
    assert k.encode_plus("a", max_length=4)["input_ids"][0].tolist()[::2] == [7, 8]


def test_golden_position_ids_follow_the_rule(golden):
    ids, pos = golden["ids"], golden["position_ids"]
    assert ids.shape == (4, 16) and pos.shape == ids.shape
    assert np.array_equal(pos, _rule(ids, 1))
    # the four kinds of row are there: no pad, right pad, left pad, pads inside the text
    live = ids != 1
    assert live[0].all() and live[1, :9].all() and not live[1, 9:].any() and not live[2, :5].any() and live[2, 5:].all()
    assert not live[3, 5] and live[3, 6] and live[3, 0] and live[3, -1]
    assert golden["mask"][2].all() and golden["mask"][3].all() and np.array_equal(golden["mask"][1], live[1])
    assert np.array_equal(_rule(np.array([[0, 9, 1, 8, 2, 1, 1, 1]]), 1), [[2, 3, 1, 4, 5, 1, 1, 1]])


def test_golden_position_gradient_rows(golden):
    g, pos = golden["g_pos"], golden["position_ids"]
    assert g.shape == (24, 128)
    assert np.abs(golden["d_pre"][2, :5]).min() > 0, "the fixture's pad tokens must carry gradient"
    assert not g[1].any(), "row pad_id of the position table received a gradient"
    assert not g[0].any() and not g[pos.max() + 1:].any()
    assert all(g[p].any() for p in range(2, pos.max() + 1))
    assert golden["g_type"].any()
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "roberta_tiny.npz")) < 1100000
