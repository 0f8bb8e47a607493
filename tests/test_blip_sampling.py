"""CPU checks of sampled captioning: the restatement of the GPU tests (tests/sampling_restatement.py) against transformers' own
TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper placed after its logits processors, ops.sampling's validation, and
what BlipCaptioner.generate refuses.  The first pins the restatement, not the device."""
import math

import pytest
import torch

transformers = pytest.importorskip("transformers")

from logits_process_restatement import hf_processors, settings  # noqa: E402
from multimodal_propaganda_meme_classification_amd import BlipCaptioner, ops  # noqa: E402
from sampling_restatement import D, draw_interval, hash32, hf_warpers, kept_set, sampling, tempered, top_p_margin, uniform  # noqa: E402
from test_blip_caption import tiny_config  # noqa: E402
from test_blip_sampling_gpu import CASES, P0, TIES, case_inputs  # noqa: E402

EOS = 102
V = 200


def _hf_kept(logits, hist, P, proc, samp):
    return hf_warpers(samp)(hist, hf_processors(P, EOS, proc)(hist, logits.clone().float())) > float("-inf")


SETTINGS = [({}, dict(temperature=0.7)), ({}, dict(temperature=1.5)), ({}, dict(top_k=1)), ({}, dict(top_k=5)), ({}, dict(top_k=V)),
            ({}, dict(top_k=V + 10)), ({}, dict(top_p=0.9)), ({}, dict(top_p=0.5)), ({}, dict(top_p=1e-6)),
            ({}, dict(temperature=1.3, top_k=20, top_p=0.8)), (dict(repetition_penalty=1.3), dict(top_k=30, top_p=0.7)),
            (dict(no_repeat_ngram_size=2, min_new_tokens=4), dict(temperature=0.7, top_p=0.95)),
            (dict(repetition_penalty=0.8, min_length=9), dict(temperature=2.0, top_k=100, top_p=0.6))]


@pytest.mark.parametrize("proc,samp", SETTINGS)
def test_kept_set_is_transformers_own(proc, samp):
    """random rows of 200 logits without ties, chosen (by their generator seed) so that no token's mass above lies within 2^-15 Z of
    top_p Z -- asserted -- : the float64 kept set equals the one transformers' float32 warpers leave finite"""
    proc, samp = settings(**proc), sampling(**samp)
    g = torch.Generator().manual_seed(17)
    done = 0
    for _ in range(10):
        hist = torch.randint(1, 7, (8, 6), generator=g)
        logits = 5 * torch.rand(8, V, generator=g) - 2.5
        logits[:, EOS] += 2.0
        far = [r for r in range(8) if top_p_margin(logits[r:r + 1], hist[r:r + 1], P0, EOS, proc, samp) >= D]
        hist, logits = hist[far], logits[far]                      # the rows of this test: none within 2^-15 Z of its boundary
        if not far:
            continue
        assert top_p_margin(logits, hist, P0, EOS, proc, samp) >= D
        x = tempered(logits, hist, P0, EOS, proc, samp)
        assert all(len(torch.unique(r[torch.isfinite(r)])) == int(torch.isfinite(r).sum()) for r in x), "no ties"
        kept = kept_set(logits, hist, P0, EOS, proc, samp)
        assert torch.equal(kept, _hf_kept(logits, hist, P0, proc, samp)), (proc, samp)
        assert kept.any(1).all()
        done += len(far)
    assert done >= 60


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_cases_meet_their_precondition(name, B):
    """the inputs of test_blip_sampling_gpu.py::test_sample_step: the top-p precondition holds, and without ties the restated kept set is
    transformers'; the intervals tile [0, 1)"""
    hist, logits, proc, samp = case_inputs(name, B)
    assert top_p_margin(logits, hist, P0, EOS, proc, samp) >= D
    kept = kept_set(logits, hist, P0, EOS, proc, samp)
    hf = _hf_kept(logits, hist, P0, proc, samp)
    rows = slice(1, None) if name in TIES else slice(None)         # row 0 holds the tie: torch.sort / topk leave it open
    assert torch.equal(kept[rows], hf[rows]), name
    if name == "a tie at the top-k threshold":
        assert torch.equal(kept[0], hf[0])                         # (transformers keeps both as well: it removes scores < kth)
    lo, hi = draw_interval(logits, hist, P0, EOS, proc, samp)
    for r in range(B):
        k = kept[r]
        assert float(lo[r][k][0]) == 0.0 and abs(float(hi[r][k][-1]) - 1) < 1e-12
        assert torch.allclose(lo[r][k][1:], hi[r][k][:-1], rtol=0, atol=1e-15) and (hi[r][k] > lo[r][k]).all()
        assert torch.isnan(lo[r][~k]).all()


def test_uniform_restated():
    assert hash32(0) == 0 and hash32(2 ** 32 + 9) == hash32(9)
    us = {(s, r, c): uniform(s, r, c) for s in (0, 1, 2 ** 32, 2 ** 64 - 1) for r in (0, 1, 2) for c in (1, 2, 30)}
    assert len(set(us.values())) == len(us) and all(0.0 <= u < 1.0 and u * 2 ** 24 == int(u * 2 ** 24) for u in us.values())
    assert uniform(2 ** 64 + 5, 1, 2) == uniform(5, 1, 2)           # the low 64 bits of the seed


def test_ops_sampling_validation():
    s = ops.sampling()
    assert (s.temperature, s.top_k, s.top_p) == (1.0, 0, 1.0) and ops.sampling_is_neutral(s)
    s = ops.sampling(temperature=0.7, top_k=50, top_p=0.9)
    assert (s.top_k, round(s.temperature, 6), round(s.top_p, 6)) == (50, 0.7, 0.9) and not ops.sampling_is_neutral(s)
    assert not ops.sampling_is_neutral(ops.sampling(top_k=1)) and not ops.sampling_is_neutral(ops.sampling(top_p=0.5))
    assert ops.sampling(temperature=2, top_p=1).temperature == 2.0   # ints are numbers
    bad = [dict(temperature=0), dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")),
           dict(temperature=True), dict(temperature="1.0"), dict(temperature=None), dict(temperature=1e-60), dict(temperature=1e60),
           dict(top_k=-1), dict(top_k=1.0), dict(top_k=True), dict(top_k="5"), dict(top_k=None), dict(top_k=2 ** 31),
           dict(top_p=0.0), dict(top_p=-0.1), dict(top_p=1.0001), dict(top_p=float("nan")), dict(top_p=True), dict(top_p="0.9"),
           dict(top_p=None), dict(top_p=1e-60)]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.sampling(**kw)
    with pytest.raises(TypeError):
        ops.sampling_is_neutral(dict(top_k=0))
    assert math.isclose(ops.sampling(top_p=1e-6).top_p, 1e-6, rel_tol=1e-6)


@pytest.mark.parametrize("kw", [dict(do_sample=True), dict(do_sample=True, num_beams=2), dict(do_sample=True, top_k=-1),
                                dict(do_sample=True, temperature=0.0), dict(do_sample=True, top_p=0.0), dict(do_sample=True, seed="7"),
                                dict(do_sample=True, num_return_sequences=2), dict(num_return_sequences=2), dict(do_sample="yes"),
                                dict(temperature=-1.0), dict(top_p=2.0)])
def test_generate_refuses(kw):
    """on a CPU model every sampled call is refused with ValueError (the draw exists only in the HIP decode step), as are bad values of
    the new keywords, with or without do_sample"""
    cap = BlipCaptioner.from_config(tiny_config())
    with pytest.raises(ValueError):
        cap.generate(torch.zeros(1, 3, 64, 64), torch.tensor([[101, 7, 102]]), **kw)


def test_caption_wrapper_passes_the_sampling_keywords():
    from multimodal_propaganda_meme_classification_amd.kevin import BlipImageCaptioning
    cap = BlipCaptioner.from_config(tiny_config())
    c = BlipImageCaptioning(None, cap, do_sample=True, temperature=0.7, top_k=50, top_p=0.9, seed=3)
    assert c.generate_kwargs == dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.9, seed=3)
    with pytest.raises(TypeError):                                 # still one caption per image
        BlipImageCaptioning(None, cap, do_sample=True, num_return_sequences=3)
