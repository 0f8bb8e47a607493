"""CPU checks of beam-search captioning: what BlipCaptioner.generate refuses, and the restated beam step of the GPU tests
(tests/beam_restatement.py) against transformers' own helpers.  The second pins the restatement, not the device."""
import pytest
import torch

transformers = pytest.importorskip("transformers")

from beam_restatement import hf_step, initial_state, ref_step, same_finished, same_scores  # noqa: E402
from multimodal_propaganda_meme_classification_amd import BlipCaptioner  # noqa: E402
from test_blip_caption import tiny_config  # noqa: E402


@pytest.mark.parametrize("kw", [dict(num_beams=0), dict(num_beams=9), dict(num_beams=3, num_return_sequences=2),
                                dict(num_beams=3, do_sample=True), dict(num_beams=2, early_stopping="sometimes")])
def test_generate_refuses(kw):
    cap = BlipCaptioner.from_config(tiny_config())
    with pytest.raises(ValueError):
        cap.generate(torch.zeros(1, 3, 64, 64), torch.tensor([[101, 7, 102]]), **kw)


@pytest.mark.parametrize("K,lp,es", [(2, 0.0, False), (3, 1.0, False), (4, 2.0, True), (5, 1.0, "never"), (8, 1.0, True)])
def test_restatement_agrees_with_transformers_helpers(K, lp, es):
    """a whole search on random logits (float32 on both sides, no ties): tokens, parents, flags, sequences and lengths equal after
    every step, scores within float32 rounding of the two log-softmax orders (1e-5)"""
    B, V, P, cap, eos = 4, 50, 3, 12, 7
    g = torch.Generator().manual_seed(100 + K)
    prompt = torch.randint(8, V, (B, P), generator=g)
    a, b = initial_state(prompt, K, cap, 0), initial_state(prompt, K, cap, 0)
    closed_seen = False
    for col in range(P, cap):
        logits = 2.0 * torch.randn(B, K, V, generator=g)
        logits[:, :, eos] += 1.5                               # eos is often among the candidates
        a, ta, pa, ia = ref_step(logits, a, col, P, cap, lp, es, eos)
        b, tb, pb, ib = hf_step(logits, b, col, P, cap, lp, es, eos)
        live = b["run_scores"] > -1e8            # a beam at -1e9 is dead: torch.topk takes it from candidates that tie in float32
        assert torch.equal(live, a["run_scores"] > -1e8) and (live.all() or col == P or col + 1 == cap), col
        assert torch.equal(ta[live], tb[live]) and torch.equal(pa[live], pb[live]), col
        assert torch.equal(a["run_seq"][live], b["run_seq"][live]) and torch.equal(a["heur"], b["heur"]), col
        assert same_scores(a["run_scores"], b["run_scores"], 1e-5), col
        assert same_finished(a, b, 1e-5) is None, (col, same_finished(a, b, 1e-5))
        assert torch.equal(ia["closed"], ib["closed"]), col
        closed_seen = closed_seen or bool(ia["closed"].any())
        b["run_scores"] = a["run_scores"].clone()              # (keep rounding differences from piling up between the two)
        b["fin_scores"] = a["fin_scores"].clone()
    assert a["fin_flags"][:, 0].all() and closed_seen


def test_restatement_tie_rule():
    """equal logits across beams and within a beam: the lower flat index beam * V + token wins, then the lower position"""
    K, V, P, cap, eos = 2, 10, 1, 6, 9
    S = initial_state(torch.tensor([[3]]), K, cap, 0, torch.float64)
    S["run_scores"][:] = -1.0                                   # both beams alive with the same score
    logits = torch.zeros(1, K, V, dtype=torch.float64)
    logits[0, :, 4] = logits[0, :, 6] = 5.0                     # four equal best candidates: (0,4) (0,6) (1,4) (1,6)
    _, tok, par, info = ref_step(logits, S, 1, P, cap, 1.0, False, eos)
    assert tok.tolist() == [[4, 6]] and par.tolist() == [[0, 0]]
    assert info["top"][0, 0] == info["top"][0, 3]
