"""CPU checks of the captioner's logits processors: the restatement the GPU tests compare the kernels with
(tests/logits_process_restatement.py) against transformers' own processors, its two beam compositions against each other, and what
BlipCaptioner.generate validates and refuses.  The first two pin the restatement, not the device."""
import pytest
import torch

transformers = pytest.importorskip("transformers")

import beam_restatement  # noqa: E402
from logits_process_restatement import (NEUTRAL, banned_tokens, beam_hf_step, beam_ref_step, greedy_ref, hf_processors, process,  # noqa: E402
                                        repeated_ngrams, settings)
from multimodal_propaganda_meme_classification_amd import BlipCaptioner, ops  # noqa: E402
from test_blip_caption import tiny_config  # noqa: E402


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_restatement_equals_transformers_processors(n):
    """random histories over few distinct tokens (so n-grams do repeat) and random logits: the banned sets are equal and every value
    is equal exactly in float32, for each processor alone and for all four in transformers' order"""
    V, eos, P = 50, 7, 3
    g = torch.Generator().manual_seed(n)
    some_ban = some_eos = False
    for L in range(1, 13):
        hist = torch.randint(0, 6, (5, L), generator=g)
        hist[0, :] = torch.randint(0, V, (L,), generator=g)             # one row with few repeats
        scores = 3 * torch.randn(5, V, generator=g)
        for s in (settings(repetition_penalty=1.3), settings(repetition_penalty=0.8), settings(no_repeat_ngram_size=n),
                  settings(min_length=6), settings(min_new_tokens=4),
                  settings(repetition_penalty=1.2, no_repeat_ngram_size=n, min_length=5, min_new_tokens=6)):
            want = hf_processors(P, eos, s)(hist, scores.clone())
            got = process(hist, scores, P, eos, s)
            assert torch.equal(torch.isneginf(got), torch.isneginf(want)), (L, s)
            assert torch.equal(got, want), (L, s)
            some_ban = some_ban or (s["no_repeat_ngram_size"] and bool(torch.isneginf(got).any()))
            some_eos = some_eos or bool(torch.isneginf(got[:, eos]).all() and s["min_new_tokens"] and not s["no_repeat_ngram_size"])
        for r in range(5):
            row = hist[r].tolist()
            assert banned_tokens(row, n) == set(torch.isneginf(process(hist[r:r + 1], scores[r:r + 1], P, eos,
                                                                       settings(no_repeat_ngram_size=n)))[0].nonzero().flatten().tolist())
    assert some_ban and some_eos


def test_restatement_edges():
    V, eos = 20, 7
    sc = torch.linspace(-2, 2, V)[None, :].clone()
    # an id that occurs three times is penalised once; a negative value is multiplied, a positive one divided
    hist = torch.tensor([[1, 18, 1, 1]])
    out = process(hist, sc, 2, eos, settings(repetition_penalty=2.0))
    assert out[0, 1] == sc[0, 1] * 2 and out[0, 18] == sc[0, 18] / 2 and torch.equal(out[0, 2:18], sc[0, 2:18])
    # nothing is banned while the history is shorter than n; n = 1 bans every token seen
    assert banned_tokens([3, 4], 3) == set() and banned_tokens([3, 4, 3], 1) == {3, 4}
    # two matches ban two tokens; a match may overlap the tail
    assert banned_tokens([5, 6, 9, 5, 6, 8, 5, 6], 3) == {9, 8}
    assert banned_tokens([4, 4, 4], 3) == {4} and banned_tokens([4, 4], 2) == {4}
    # min_length counts the prompt, min_new_tokens does not
    for L, ml, mn, banned in ((4, 5, 0, True), (5, 5, 0, False), (4, 0, 2, True), (5, 0, 2, False), (5, 3, 3, True)):
        out = process(torch.zeros(1, L, dtype=torch.int64), sc, 3, eos, settings(min_length=ml, min_new_tokens=mn))
        assert bool(torch.isneginf(out[0, eos])) == banned, (L, ml, mn)
    assert repeated_ngrams([1, 2, 3, 1, 2], 2) == {(1, 2)} and repeated_ngrams([1, 2, 3, 1, 2], 3) == set()
    tok, _ = greedy_ref(sc, torch.tensor([[19, 18]]), 1, eos, settings(no_repeat_ngram_size=1))
    assert tok.tolist() == [17]


@pytest.mark.parametrize("K,s", [(2, settings(repetition_penalty=1.3)), (3, settings(no_repeat_ngram_size=2, min_new_tokens=4)),
                                 (3, settings(repetition_penalty=1.2, no_repeat_ngram_size=3, min_length=8))])
def test_beam_compositions_agree(K, s):
    """a whole search with processors on random logits, tokens from a small alphabet so that bans bite: the composition with
    ref_step (float32 here) and the one with transformers' helpers and processors agree as test_blip_beam.py asks of the plain steps"""
    B, V, P, cap, eos = 3, 50, 3, 14, 7
    g = torch.Generator().manual_seed(200 + K)
    prompt = torch.randint(8, 14, (B, P), generator=g)
    a, b = beam_restatement.initial_state(prompt, K, cap, 0), beam_restatement.initial_state(prompt, K, cap, 0)
    banned_any = False
    for col in range(P, cap):
        logits = 0.3 * torch.randn(B, K, V, generator=g)
        logits[:, :, 8:14] += 3.0                               # the search stays within six tokens: n-grams repeat
        logits[:, :, eos] += 2.0
        a, ta, pa, ia = beam_ref_step(logits, a, col, P, cap, 1.0, False, eos, s)
        b, tb, pb, ib = beam_hf_step(logits, b, col, P, cap, 1.0, False, eos, s)
        live = b["run_scores"] > -1e8
        assert torch.equal(live, a["run_scores"] > -1e8), col
        assert torch.equal(ta[live], tb[live]) and torch.equal(pa[live], pb[live]), col
        assert torch.equal(a["run_seq"][live], b["run_seq"][live]) and torch.equal(a["heur"], b["heur"]), col
        assert beam_restatement.same_scores(a["run_scores"], b["run_scores"], 1e-5), col
        assert beam_restatement.same_finished(a, b, 1e-5) is None, (col, beam_restatement.same_finished(a, b, 1e-5))
        b["run_scores"], b["fin_scores"] = a["run_scores"].clone(), a["fin_scores"].clone()
        n = s["no_repeat_ngram_size"]
        if n:
            for r in a["run_seq"][live].tolist():
                assert not repeated_ngrams(r[:col + 1], n), (col, r)
            banned_any = banned_any or any(banned_tokens(r[:col + 1], n) for r in a["run_seq"][live].tolist())
        if s["min_new_tokens"] or s["min_length"]:
            f = a["fin_flags"]
            assert (a["fin_len"][f] >= max(s["min_new_tokens"], s["min_length"] - P) + 1).all(), col      # eos is the token after them
    assert a["fin_flags"][:, 0].all() and (banned_any or not s["no_repeat_ngram_size"])


def test_neutral_composition_is_the_plain_step():
    B, K, V, P, cap, eos = 2, 3, 40, 2, 8, 5
    g = torch.Generator().manual_seed(9)
    S = beam_restatement.initial_state(torch.randint(6, V, (B, P), generator=g), K, cap, 0, torch.float64)
    logits = torch.randn(B, K, V, generator=g, dtype=torch.float64)
    a = beam_ref_step(logits, S, P, P, cap, 1.0, False, eos, NEUTRAL)
    b = beam_restatement.ref_step(logits, S, P, P, cap, 1.0, False, eos)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and float((a[0]["run_scores"] - b[0]["run_scores"]).abs().max()) < 1e-12


# ---- what generate validates ----------------------------------------------------------------------------------------------------

BAD = [dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("inf")), dict(repetition_penalty=float("nan")),
       dict(repetition_penalty="1.2"), dict(repetition_penalty=True), dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=2.0),
       dict(min_length=-3), dict(min_length=True), dict(min_new_tokens=-1), dict(min_new_tokens=1.5), dict(num_return_sequences=0),
       dict(num_return_sequences=2), dict(num_beams=2, num_return_sequences=3), dict(num_beams=3, num_return_sequences=1.0)]


@pytest.mark.parametrize("kw", BAD)
def test_generate_refuses_bad_values(kw):
    cap = BlipCaptioner.from_config(tiny_config())
    with pytest.raises(ValueError):
        cap.generate(torch.zeros(1, 3, 64, 64), torch.tensor([[101, 7, 102]]), **kw)


@pytest.mark.parametrize("kw", [dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2), dict(min_length=4), dict(min_new_tokens=1),
                                dict(num_beams=3, num_return_sequences=2), dict(num_beams=2, repetition_penalty=1.1)])
def test_generate_refuses_processors_off_the_device(kw):
    """valid values, but the model and batch are on the CPU: the processors and the n-best return exist in the device step only"""
    cap = BlipCaptioner.from_config(tiny_config())
    with pytest.raises(ValueError):
        cap.generate(torch.zeros(1, 3, 64, 64), torch.tensor([[101, 7, 102]]), **kw)


def test_logits_process_settings():
    p = ops.logits_process(1.25, 3, 4, 5)
    assert (p.repetition_penalty, p.no_repeat_ngram_size, p.min_length, p.min_new_tokens) == (1.25, 3, 4, 5)
    assert ops.process_is_neutral(None) and ops.process_is_neutral(ops.logits_process()) and not ops.process_is_neutral(p)
    assert not ops.process_is_neutral(ops.logits_process(min_new_tokens=1))
    for kw in (dict(repetition_penalty=0), dict(no_repeat_ngram_size=-1), dict(min_length=2 ** 31), dict(min_new_tokens="3")):
        with pytest.raises(ValueError):
            ops.logits_process(**kw)
