"""GPU checks of the captioner's logits processors (repetition penalty, n-gram ban, minimum lengths) and of the n-best return:
mh_greedy_step_processed against the float32 restatement, mh_beam_step_processed against the float64 one
(tests/logits_process_restatement.py, pinned on the CPU by test_blip_processors.py), and BlipCaptioner.generate with these keywords
against a replay through transformers' own processors and helpers and against BlipForConditionalGeneration.generate."""
import pytest
import torch

transformers = pytest.importorskip("transformers")

from beam_restatement import initial_state, same_finished, same_scores  # noqa: E402
from conftest import parity_log  # noqa: E402
from logits_process_restatement import (NEUTRAL, beam_hf_step, beam_ref_step, greedy_ref, hf_processors, process, repeated_ngrams,  # noqa: E402
                                        settings)
from multimodal_propaganda_meme_classification_amd import ops  # noqa: E402
from test_blip_beam_gpu import FILL, PROMPT, TOL, _from_device, _mid_state, _to_device  # noqa: E402
from test_blip_caption import tiny_config  # noqa: E402
from test_blip_caption_gpu import _pair, _pix  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EOS, PAD = 102, 0
V, VP = 200, 256


# ---- 1. / 2. mh_greedy_step_processed against the float32 restatement ----------------------------------------------------------------

def _greedy_kernel(hist, logits, P, cap, s, Vp=VP):
    """one step after the history hist int64 [B, col] on f32 logits [B, V']: (tokens [B], finished [B], state words)"""
    B, col = hist.shape
    Vv = logits.shape[1]
    full = torch.full((B, Vp), 1e30)                     # a padded column would win every argmax if it were read
    full[:, :Vv] = logits
    out = torch.full((B, cap), PAD, dtype=torch.int64)
    out[:, :col] = hist
    out = out.to(DEV)
    nxt = torch.zeros(B, dtype=torch.int64, device=DEV)
    fin = torch.zeros(B, dtype=torch.int32, device=DEV)
    st = torch.tensor([col - 1, 0, 0, 0], dtype=torch.int32, device=DEV)
    ops.greedy_step(full.to(DEV), Vv, out, nxt, fin, st, P, EOS, PAD, process=ops.logits_process(**s))
    out = out.cpu()
    assert torch.equal(out[:, col], nxt.cpu()) and torch.equal(out[:, :col], hist) and (out[:, col + 1:] == PAD).all()
    return nxt.cpu(), fin.cpu(), st.cpu().tolist()


def _greedy_check(what, hist, logits, P, cap, s, rounds=3, Vp=VP):
    """the kernel's token equals the float32 restatement's -- exactly: the processors are one f32 multiply or divide per value --
    `rounds` times: after each round the winners' logits drop below the row, so the runners-up are compared as well"""
    logits = logits.clone()
    first = None
    for _ in range(rounds):
        got, fin, state = _greedy_kernel(hist, logits, P, cap, s, Vp)
        want, _ = greedy_ref(logits, hist, P, EOS, s)
        assert torch.equal(got, want), (what, got.tolist(), want.tolist())
        assert fin.tolist() == [int(t == EOS) for t in want.tolist()], what
        assert state[:3] == [hist.shape[1], 0, sum(fin.tolist())], (what, state)
        first = got if first is None else first
        logits[torch.arange(len(got)), got] = float(logits.min()) - 1.0
    return first


def _rows(row0, B, g, lo=1, hi=100):
    """row0 (the constructed history) plus B - 1 random histories of its length over few tokens, so that their n-grams repeat too"""
    L = len(row0)
    h = torch.randint(lo, min(hi, lo + 6), (B, L), generator=g)
    h[0] = torch.tensor(row0)
    return h


def _logits(B, g, over, negative=False, Vv=V):
    x = 5 * torch.rand(B, Vv, generator=g) - 2.5                # no ties
    if negative:
        x = -3.0 - x.abs()
    for t, v in over.items():
        x[0, t] = v
    return x


BOS = 150
# name: (history of row 0, prompt length, {token: logit} of row 0, all-negative logits?, settings, the token row 0 must pick)
GREEDY_CASES = {
    "a penalised positive logit": ([BOS, 7, 8, 40], 3, {40: 9.0, 41: 8.0}, False, dict(repetition_penalty=1.2), 41),
    "a penalised negative logit": ([BOS, 7, 8, 40], 3, {40: -0.5, 41: -0.55}, True, dict(repetition_penalty=1.2), 41),
    "an id three times in the history is penalised once": ([BOS, 7, 8, 40, 9, 40, 40], 3, {40: 9.0, 41: 7.0}, False, dict(repetition_penalty=1.2), 40),
    "a prompt token is penalised": ([BOS, 7, 8, 30], 3, {7: 9.0, 41: 8.0}, False, dict(repetition_penalty=1.2), 41),
    "a penalty below 1 rewards": ([BOS, 7, 8, 40], 3, {40: 8.0, 41: 9.0}, False, dict(repetition_penalty=0.8), 40),
    "n = 1": ([BOS, 7, 8, 40], 3, {40: 9.0, 41: 8.0}, False, dict(no_repeat_ngram_size=1), 41),
    "n = 2": ([BOS, 7, 8, 20, 21, 20], 3, {21: 9.0, 41: 8.0}, False, dict(no_repeat_ngram_size=2), 41),
    "n = 3": ([BOS, 7, 8, 20, 21, 22, 20, 21], 3, {22: 9.0, 41: 8.0}, False, dict(no_repeat_ngram_size=3), 41),
    "a history shorter than n - 1": ([BOS], 1, {40: 9.0, 41: 8.0}, False, dict(no_repeat_ngram_size=3), 40),
    "a history of n - 1 tokens": ([BOS, 40], 1, {40: 9.0, 41: 8.0}, False, dict(no_repeat_ngram_size=3), 40),
    "a match that starts inside the prompt": ([BOS, 7, 8, 9, 7, 8], 3, {9: 9.0, 41: 8.0}, False, dict(no_repeat_ngram_size=3), 41),
    "two matches ban two tokens": ([BOS, 20, 21, 30, 20, 21, 31, 20, 21], 3, {30: 9.0, 31: 8.5, 32: 8.0}, False, dict(no_repeat_ngram_size=3), 32),
    "a match overlapping the tail": ([BOS, 7, 8, 4, 4, 4], 3, {4: 9.0, 41: 8.0}, False, dict(no_repeat_ngram_size=3), 41),
    "eos at col = min_length - 1": ([BOS, 7, 8, 30, 31], 3, {EOS: 9.0, 41: 8.0}, False, dict(min_length=6), 41),
    "eos at col = min_length": ([BOS, 7, 8, 30, 31, 32], 3, {EOS: 9.0, 41: 8.0}, False, dict(min_length=6), EOS),
    "eos one short of min_new_tokens": ([BOS, 7, 8, 30, 31], 3, {EOS: 9.0, 41: 8.0}, False, dict(min_new_tokens=3), 41),
    "eos at min_new_tokens": ([BOS, 7, 8, 30, 31, 32], 3, {EOS: 9.0, 41: 8.0}, False, dict(min_new_tokens=3), EOS),
    "both minimums, min_new_tokens the stricter": ([BOS, 7, 8, 30, 31, 32], 3, {EOS: 9.0, 41: 8.0}, False, dict(min_length=5, min_new_tokens=4), 41),
    "both minimums, min_length the stricter": ([BOS, 7, 8, 30, 31, 32], 3, {EOS: 9.0, 41: 8.0}, False, dict(min_length=8, min_new_tokens=2), 41),
    "both minimums reached": ([BOS, 7, 8, 30, 31, 32], 3, {EOS: 9.0, 41: 8.0}, False, dict(min_length=6, min_new_tokens=3), EOS),
    "the top token penalised and banned": ([BOS, 7, 8, 40], 3, {40: 9.0, 41: 8.0}, False, dict(repetition_penalty=1.2, no_repeat_ngram_size=1), 41),
}


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", list(GREEDY_CASES))
def test_greedy_step_processed(name, B):
    row0, P, over, negative, s, expect = GREEDY_CASES[name]
    g = torch.Generator().manual_seed(len(name) + B)
    hist = _rows(row0, B, g)
    hist[:, 0] = BOS
    first = _greedy_check(name, hist, _logits(B, g, over, negative), P, 12, settings(**s))
    assert int(first[0]) == expect, (name, first.tolist())
    # without the processors row 0 picks its largest logit: the case does show the processor
    plain, _, _ = _greedy_kernel(hist, _logits(B, torch.Generator().manual_seed(len(name) + B + 1000), over, negative), P, 12, NEUTRAL)
    assert int(plain[0]) == max(over, key=over.get), name


EDGE_IDS = [0, 31, 32, 63, 64, V - 1]


@pytest.mark.parametrize("s", [dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=1), dict(no_repeat_ngram_size=2, repetition_penalty=1.5)])
def test_greedy_bitmap_word_edges(s):
    """bits 0 and 31 of a word, the first and last word (V = 200 leaves a partial one): the id is penalised or banned, its neighbour,
    one bit further, is not"""
    g = torch.Generator().manual_seed(3)
    B = len(EDGE_IDS)
    hist = torch.tensor([[BOS, 7, t, 9, t] for t in EDGE_IDS])          # (t, 9) then t again: n = 2 bans 9 ... and n = 1 bans t
    x = 5 * torch.rand(B, V, generator=g) - 2.5
    near = [t + 1 if t + 1 < V else t - 1 for t in EDGE_IDS]
    for r, (t, nb) in enumerate(zip(EDGE_IDS, near)):
        x[r, t], x[r, nb], x[r, 9] = 9.0, 8.5, 8.8
    first = _greedy_check(f"edges {s}", hist, x, 2, 12, settings(**s), rounds=4)
    # t and 9 are both in the history: penalised (to 7.5 and 7.33, or 6 and 5.87) or banned, below the neighbour's untouched 8.5
    assert first.tolist() == near


def test_greedy_history_of_two_trips():
    """cap = 300, col = 290: the history takes two trips of the 256 threads; one earlier occurrence of the tail lies in each"""
    g = torch.Generator().manual_seed(4)
    B, col, cap = 2, 290, 300
    hist = torch.randint(0, 190, (B, col), generator=g)
    hist[0, 10:13] = torch.tensor([198, 199, 50])
    hist[0, 270:273] = torch.tensor([198, 199, 51])
    hist[0, 288:290] = torch.tensor([198, 199])
    hist[0, 280] = 195                                                   # seen only beyond position 256
    x = _logits(B, g, {50: 9.0, 51: 8.8, 195: 8.7, 196: 8.0})
    s = settings(no_repeat_ngram_size=3, repetition_penalty=1.2)
    first = _greedy_check("two trips", hist, x, 3, cap, s, rounds=4)
    assert int(first[0]) == 196
    assert int(_greedy_kernel(hist, x, 3, cap, NEUTRAL)[0][0]) == 50


def test_greedy_large_vocabulary():
    Vv, Vp = 30524, 30592
    g = torch.Generator().manual_seed(5)
    hist = torch.randint(0, Vv, (2, 9), generator=g)
    hist[0] = torch.tensor([30522, 5, 6, 30523, 30500, 0, 7, 30523, 30500])
    x = 5 * torch.rand(2, Vv, generator=g) - 2.5
    x[0, 0], x[0, 30523], x[0, 30500], x[0, 17] = 9.0, 8.8, 8.7, 8.0
    first = _greedy_check("V=30524", hist, x, 3, 12, settings(no_repeat_ngram_size=3, repetition_penalty=1.3), rounds=4, Vp=Vp)
    assert int(first[0]) == 17


def test_greedy_processed_refusals():
    g = torch.Generator().manual_seed(6)
    x = torch.rand(1, 40000, generator=g).to(DEV)
    out = torch.zeros(1, 8, dtype=torch.int64, device=DEV)
    nxt, fin, st = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):                                      # the bitmaps of 40000 tokens do not fit
        ops.greedy_step(x, 40000, out, nxt, fin, st, 1, EOS, PAD, process=ops.logits_process(no_repeat_ngram_size=2))
    ops.greedy_step(x, 40000, out, nxt, fin, st, 1, EOS, PAD, process=ops.logits_process())          # neutral: the plain kernel
    assert st.tolist()[0] == 1
    with pytest.raises(TypeError):
        ops.greedy_step(x, 40000, out, nxt, fin, st, 1, EOS, PAD, process=dict(no_repeat_ngram_size=2))


# ---- 3. mh_beam_step_processed against the float64 restatement ------------------------------------------------------------------------

def _margin(logits, S, col, P, s):
    """float64: the smallest lead of one of the best 2K candidates of an image over the next candidate (the 2K-th over the first
    one not selected included)"""
    B, K, Vv = logits.shape
    x = logits.double()
    m = x.max(-1, keepdim=True)[0]
    logp = (x - m) - torch.log(torch.exp(x - m).sum(-1, keepdim=True))
    y = process(S["run_seq"][:, :, :col].reshape(B * K, col), logp.reshape(B * K, Vv), P, EOS, s).reshape(B, K, Vv)
    acc = (y + S["run_scores"].double()[:, :, None]).reshape(B, K * Vv)
    top = acc.sort(1, descending=True)[0][:, :2 * K + 1]
    assert torch.isfinite(top).all()
    return float((top[:, :-1] - top[:, 1:]).min())


def _beam_case(what, logits, S, col, P, cap, s, lp=1.0, es=False, bs=None):
    """test_blip_beam_gpu._run_kernel_case's checks with the processors on both sides; bs: continue on this device state"""
    B, K, Vv = logits.shape
    s = settings(**s)
    margin = _margin(logits, S, col, P, s)
    assert margin >= 1e-3, (what, margin)           # no case passes by luck or fails by a near-tie
    full = torch.full((B * K, VP), 1e30)
    full[:, :Vv] = logits.reshape(B * K, Vv)
    bs = _to_device(S, B, K, cap, col) if bs is None else bs
    ops.beam_step(full.to(DEV), Vv, bs, P, lp, es, EOS, process=ops.logits_process(**s))
    got, tok, par, state = _from_device(bs)
    want, wtok, wpar, info = beam_ref_step(logits.double(), S, col, P, cap, lp, es, EOS, s)
    real = want["run_scores"] > -1e8
    err = float((got["run_scores"].double() - want["run_scores"])[real].abs().max()) if real.any() else 0.0
    parity_log(f"beam_step processed {what} B={B} K={K}: float64 margin {margin:.3e}, max|running score err| {err:.3e}")
    assert torch.equal(tok, wtok) and torch.equal(par, wpar), (what, tok.tolist(), wtok.tolist(), par.tolist(), wpar.tolist())
    assert torch.equal(got["run_seq"], want["run_seq"]) and torch.equal(got["heur"], want["heur"]), what
    assert same_scores(got["run_scores"], want["run_scores"], TOL), what
    assert same_finished(got, want, TOL) is None, (what, same_finished(got, want, TOL))
    assert torch.equal(got["fin_seq"], want["fin_seq"]) and torch.equal(got["fin_len"], want["fin_len"]), what
    assert state == [col, 0, 0, int(bool(info["closed"].all()))], (what, state)
    assert not torch.isnan(got["run_scores"]).any() and not torch.isnan(got["fin_scores"]).any(), what
    return got, want, tok, par, bs


def _ranked_rows(B, K, g, tops):
    """uniform noise in [-1, 1) with, per beam, the given {token: logit}"""
    x = 2 * torch.rand(B, K, V, generator=g) - 1
    for k, over in enumerate(tops):
        for t, v in over.items():
            x[:, k, t] = v
    return x


def _state_with(B, K, cap, P, col, g, beam0_tail):
    """a search in progress whose beams are 20 apart (every best candidate comes from beam 0), beam 0's last tokens as given"""
    S = _mid_state(B, K, cap, P, col, g, V, spread=20.0)
    S["run_seq"][:, :, P:col] = torch.randint(110, 140, (B, K, col - P), generator=g)          # away from the tokens the cases use
    S["run_seq"][:, 0, col - len(beam0_tail):col] = torch.tensor(beam0_tail)
    return S


@pytest.mark.parametrize("B,K", [(1, 2), (3, 3), (3, 8)])
def test_beam_step_penalty_acts_on_log_probabilities(B, K):
    P, cap, col = 3, 12, 6
    g = torch.Generator().manual_seed(30 + K)
    S = _state_with(B, K, cap, P, col, g, [10, 11])
    tops = [{10 + j: 12.0 - 0.5 * j for j in range(2 * K + 2)}] + [{}] * (K - 1)
    x = _ranked_rows(B, K, g, tops)
    s = dict(repetition_penalty=3.0)
    _, _, tok, par, _ = _beam_case("penalty", x, S, col, P, cap, s)
    _, ptok, _, _ = beam_ref_step(x.double(), S, col, P, cap, 1.0, False, EOS, NEUTRAL)
    assert (ptok[:, 0] == 10).all() and (tok[:, 0] == 12).all() and (par == 0).all()      # 10 and 11 (log p < 0, times 3) fall behind


@pytest.mark.parametrize("B,K", [(1, 2), (3, 3), (3, 8)])
def test_beam_step_bans_the_images_best_candidate(B, K):
    P, cap, col = 3, 12, 7
    g = torch.Generator().manual_seed(40 + K)
    S = _state_with(B, K, cap, P, col, g, [60, 10, 77, 60])                # after 60 came 10: n = 2 bans 10
    tops = [{10 + j: 12.0 - 0.5 * j for j in range(2 * K + 2)}] + [{}] * (K - 1)
    x = _ranked_rows(B, K, g, tops)
    got, _, tok, _, _ = _beam_case("banned best", x, S, col, P, cap, dict(no_repeat_ngram_size=2))
    assert (tok[:, 0] == 11).all() and not (tok == 10).any() and not (got["run_seq"][:, :, col] == 10).any()


@pytest.mark.parametrize("B,K", [(1, 2), (3, 3)])
def test_beam_step_eos_banned_under_min_new_tokens(B, K):
    P, cap, col = 3, 12, 6
    g = torch.Generator().manual_seed(50 + K)
    S = _state_with(B, K, cap, P, col, g, [61])
    tops = [{EOS: 13.0, **{10 + j: 12.0 - 0.5 * j for j in range(2 * K + 2)}}] + [{EOS: 5.0}] * (K - 1)
    x = _ranked_rows(B, K, g, tops)
    got, _, tok, _, _ = _beam_case("eos banned", x, S, col, P, cap, dict(min_new_tokens=4))            # 3 new tokens so far
    assert not got["fin_flags"].any() and not (tok == EOS).any()
    got, _, _, _, _ = _beam_case("eos free", x, S, col, P, cap, dict(min_new_tokens=3))
    assert got["fin_flags"][:, 0].all() and (got["fin_seq"][:, 0, col] == EOS).all()
    got, _, _, _, _ = _beam_case("eos banned by min_length", x, S, col, P, cap, dict(min_length=7, min_new_tokens=1))
    assert not got["fin_flags"].any()


def test_beam_step_ban_follows_the_parent():
    """two consecutive steps on the device state: in the first, beams 0 and 1 both continue old beam 0 (with 10 and 11); in the
    second, beam 1's history is old beam 0's plus 11 -- where 11 was followed by 77 -- so n = 2 bans 77 for beam 1, its best token"""
    B, K, P, cap, col = 3, 3, 3, 12, 6
    g = torch.Generator().manual_seed(60)
    S = _state_with(B, K, cap, P, col, g, [11, 77, 62])
    s = dict(no_repeat_ngram_size=2)
    x1 = _ranked_rows(B, K, g, [{10 + j: 12.0 - 0.5 * j for j in range(2 * K + 2)}] + [{}] * (K - 1))
    _, S1, tok, par, bs = _beam_case("parent step 1", x1, S, col, P, cap, s)
    assert tok[:, :2].tolist() == [[10, 11]] * B and (par == 0).all()
    assert (S1["run_seq"][:, 1, col - 3:col + 1] == torch.tensor([11, 77, 62, 11])).all()
    x2 = _ranked_rows(B, K, g, [{30: 6.0, 31: 5.5}, {77: 12.0, 78: 9.0, 79: 8.5}, {}])
    _, ptok, ppar, _ = beam_ref_step(x2.double(), S1, col + 1, P, cap, 1.0, False, EOS, NEUTRAL)
    assert ((ptok == 77) & (ppar == 1)).any(1).all(), "without the ban (beam 1, 77) is among the new beams"
    got, _, tok, par, _ = _beam_case("parent step 2", x2, S1, col + 1, P, cap, s, bs=bs)
    assert not (tok == 77).any() and ((tok == 78) & (par == 1)).any(1).all()


def test_beam_step_processed_refusals_and_neutral():
    B, K, P = 1, 8, 3
    g = torch.Generator().manual_seed(70)
    cap = V - 2 * K                                  # 2K + cap + 1 = V + 1: one token short
    prompt = torch.randint(1, 100, (B, P), generator=g)
    bs = ops.beam_state(B, K, cap, prompt, PAD, DEV)
    x = torch.randn(B * K, VP, generator=g).to(DEV)
    with pytest.raises(ValueError):
        ops.beam_step(x, V, bs, P, 1.0, False, EOS, process=ops.logits_process(repetition_penalty=1.1))
    assert bs["state"].tolist() == [0, 0, 0, 0]
    ops.beam_step(x, V, bs, P, 1.0, False, EOS, process=ops.logits_process())              # neutral: the plain entry point takes it
    assert bs["state"].tolist()[0] == 1
    bs2 = ops.beam_state(B, K, cap - 1, prompt, PAD, DEV)                                 # one column fewer: accepted
    ops.beam_step(x, V, bs2, P, 1.0, False, EOS, process=ops.logits_process(repetition_penalty=1.1))
    assert bs2["state"].tolist()[0] == 1
    # neutral settings through the processed step equal the plain step bit for bit
    S = _mid_state(2, 3, 12, P, 6, g, V)
    lg = torch.full((6, VP), 1e30)
    lg[:, :V] = 3 * torch.randn(6, V, generator=g)
    a, b = _to_device(S, 2, 3, 12, 6), _to_device(S, 2, 3, 12, 6)
    ops.beam_step(lg.to(DEV), V, a, P, 1.0, False, EOS)
    ops.beam_step(lg.to(DEV), V, b, P, 1.0, False, EOS, process=ops.logits_process(1.0, 0, 0, 0))
    for n in ("next_ids", "parents", "run_scores", "run_seq", "fin_seq", "fin_scores", "fin_flags", "fin_len", "heur", "state"):
        assert torch.equal(a[n], b[n]), n


# ---- 4. BlipCaptioner.generate --------------------------------------------------------------------------------------------------------

# The reference model runs in float32, the captioner in 16 bits: its logits differ by up to a few percent of their spread, which moves
# a greedy or beam decision wherever the reference's lead is that small.  These seeds are models whose decisions, in every case below,
# have leads beyond that error, so the captions can be compared token for token; SHOW_SEED is a model whose plain captions loop and
# end early (it is compared with transformers only in fp16, where it is SEEDS["fp16"]).
SEEDS = {"fp16": 17, "bf16": 13}
SHOW_SEED = 17
NB, MAX_NEW = 4, 16
S1 = dict(repetition_penalty=1.2, no_repeat_ngram_size=2, min_new_tokens=8)
S2 = dict(no_repeat_ngram_size=3, min_length=12)
_models = {}


def _model(dtype, seed=None):
    seed = SEEDS[dtype] if seed is None else seed
    if (dtype, seed) not in _models:
        _models[(dtype, seed)] = _pair(tiny_config(), dtype, seed=seed, eos_boost=1.0)
    return _models[(dtype, seed)]


def _prompt(B=NB):
    return torch.tensor([PROMPT] * B)


_hf = {}


def _hf_generate(ref, K, n, kw):
    key = (id(ref), K, n, tuple(sorted(kw.items())))
    if key not in _hf:
        with torch.no_grad():
            _hf[key] = ref.generate(pixel_values=_pix(NB, 64), input_ids=_prompt(), max_new_tokens=MAX_NEW, num_beams=K,
                                    num_return_sequences=n, **kw)
    return _hf[key]


def _greedy_replay(ours, pix, kw, what):
    """generate with the trace hook, then every step's own logits through transformers' LogitsProcessorList and an argmax: the same
    tokens step by step.  Returns the output and, per row and column, the float64 lead of the chosen token over the runner-up."""
    B = pix.shape[0]
    trace = []
    out = ours.generate(pix, _prompt(B), max_new_tokens=MAX_NEW, poll_every=1, _trace=trace, **kw).cpu()
    P = len(PROMPT) - 1
    ids = _prompt(B)
    ids[:, 0] = ours.text_cfg["bos_token_id"]
    hist = ids[:, :P].clone()
    procs = hf_processors(P, EOS, kw)
    fin = torch.zeros(B, dtype=torch.bool)
    gaps = torch.full((B, P + MAX_NEW), float("inf"), dtype=torch.float64)
    for i, tr in enumerate(trace):
        col = i + 1
        chosen = tr["next_ids"].cpu()
        if col < P:
            assert torch.equal(chosen, ids[:, col]), (what, col)
            continue
        sc = procs(hist, tr["logits"].cpu().float().clone())
        want = sc.argmax(-1)
        want[fin] = PAD
        assert torch.equal(chosen, want), (what, col, chosen.tolist(), want.tolist())
        top2 = sc.double().topk(2).values
        gaps[:, col] = torch.where(torch.isfinite(top2[:, 1]), top2[:, 0] - top2[:, 1], torch.tensor(float("inf"), dtype=torch.float64))
        hist = torch.cat([hist, chosen[:, None]], 1)
        fin |= chosen == EOS
    assert torch.equal(out, hist[:, :out.shape[1]]), what
    return out, gaps


def _beam_replay(ours, pix, K, n, kw, what):
    """test_blip_beam_gpu._replay with transformers' processors between its log-softmax and the beam scores (beam_hf_step), and the
    n best finished beams at the end.  Returns the output and, per image and column, the smallest float64 lead among the best 2K."""
    B = pix.shape[0]
    trace = []
    out = ours.generate(pix, _prompt(B), max_new_tokens=MAX_NEW, num_beams=K, num_return_sequences=n, poll_every=1, _trace=trace, **kw).cpu()
    P, Vv = len(PROMPT) - 1, ours.text_cfg["vocab_size"]
    cap = P + MAX_NEW
    ids = _prompt(B)
    ids[:, 0] = ours.text_cfg["bos_token_id"]
    S = initial_state(ids[:, :P], K, cap, FILL)
    gaps = torch.full((B, cap), float("inf"), dtype=torch.float64)
    for i, tr in enumerate(trace):
        col = i + 1
        if col < P:
            assert tr["next_ids"].view(B, K).cpu().tolist() == [[int(ids[b, col])] * K for b in range(B)]
            continue
        S, tok, par, info = beam_hf_step(tr["logits"].cpu().view(B, K, Vv), S, col, P, cap, 1.0, False, EOS, kw)
        dev = dict(run_scores=tr["run_scores"].cpu().view(B, K), run_seq=tr["run_seq"].cpu().view(B, K, cap).long(),
                   fin_seq=tr["fin_seq"].cpu().view(B, K, cap).long(), fin_scores=tr["fin_scores"].cpu().view(B, K),
                   fin_flags=tr["fin_flags"].cpu().view(B, K).bool(), fin_len=tr["fin_len"].cpu().view(B, K).long(), heur=tr["heur"].cpu().bool())
        live = S["run_scores"] > -1e8
        assert torch.equal(live, dev["run_scores"] > -1e8), (what, col)
        assert torch.equal(tr["next_ids"].cpu().view(B, K)[live], tok[live]), (what, col, "running tokens")
        assert torch.equal(tr["parents"].cpu().view(B, K).long()[live], par[live]), (what, col, "parents")
        assert torch.equal(dev["run_seq"][live], S["run_seq"][live]) and torch.equal(dev["heur"], S["heur"]), (what, col)
        assert same_scores(dev["run_scores"], S["run_scores"], TOL), (what, col)
        assert same_finished(dev, S, TOL) is None, (what, col, same_finished(dev, S, TOL))
        top = info["top"].double()
        d = top[:, :-1] - top[:, 1:]
        gaps[:, col] = torch.where(torch.isfinite(d), d, torch.tensor(float("inf"), dtype=torch.float64)).min(1)[0]
        S["run_scores"], S["fin_scores"] = dev["run_scores"].clone(), dev["fin_scores"].clone()
    assert int(trace[-1]["state"][3]) == 1 and S["fin_flags"][:, 0].all(), what
    L = P + int(S["fin_len"][:, :n].max())
    held = S["fin_flags"][:, :n]
    got = out.view(B, n, -1)
    assert got.shape[2] == L, (what, got.shape, L)
    assert torch.equal(got[held], S["fin_seq"][:, :n, :L][held]), what
    empty = torch.cat([ids[:, :P], torch.full((B, L - P), FILL)], 1)[:, None, :].expand(B, n, L)
    assert torch.equal(got[~held], empty[~held]), (what, "a slot without a finished beam is the prompt and padding")
    return out, gaps


_near_ties = {"steps": 0, "accepted": 0}


def _against_transformers(got, want, gaps, rows_per_image, what):
    """equal to BlipForConditionalGeneration.generate with the same keywords; a row may differ only from a step on where the replay
    shows a float64 lead below 1e-3, and over all cases at most 1 step in 20 may be such a step"""
    n = min(got.shape[1], want.shape[1])
    P = len(PROMPT) - 1
    _near_ties["steps"] += got.shape[0] * (n - P)
    assert got.shape[0] == want.shape[0], (what, got.shape, want.shape)
    for r in range(got.shape[0]):
        a, b = got[r].tolist(), want[r].tolist()
        if a == b:
            continue
        diff = [c for c in range(n) if a[c] != b[c]]
        c = diff[0] if diff else n - 1                 # equal up to the shorter length: the step that ended one of them
        lead = float(gaps[r // rows_per_image, :c + 1].min())
        parity_log(f"{what}: row {r} leaves transformers' at column {c}; smallest replay lead up to there {lead:.3e}")
        assert lead < 1e-3, (what, r, c, lead, a, b)
        _near_ties["accepted"] += 1
    if got.shape == want.shape and torch.equal(got, want):
        parity_log(f"{what}: equal to transformers' generate {tuple(got.shape)}")
    assert _near_ties["accepted"] * 20 <= _near_ties["steps"], _near_ties


def _caption(row, P):
    """the row up to and including its first eos after the prompt (what follows is padding)"""
    row = row.tolist()
    return row[:row.index(EOS, P) + 1] if EOS in row[P:] else row


def _properties(out, kw, what):
    P = len(PROMPT) - 1
    n = kw.get("no_repeat_ngram_size", 0)
    for r in out:
        c = _caption(r, P)
        if n:
            assert not repeated_ngrams(c, n), (what, c)
        if EOS in c[P:]:
            assert len(c) - 1 >= kw.get("min_length", 0) and len(c) - 1 - P >= kw.get("min_new_tokens", 0), (what, c)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("kw", [S1, S2], ids=["S1", "S2"])
def test_generate_greedy_with_processors(dtype, kw):
    ref, ours = _model(dtype)
    pix = _pix(NB, 64).to(DEV)
    what = f"greedy {dtype} {kw}"
    out, gaps = _greedy_replay(ours, pix, kw, what)
    _properties(out, kw, what)
    _against_transformers(out, _hf_generate(ref, 1, 1, kw), gaps, 1, what)
    eager = ours.generate(pix, _prompt(), max_new_tokens=MAX_NEW, graph=False, **kw).cpu()
    assert torch.equal(out, eager), "graph replay must equal graph=False"


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("kw", [S1, S2], ids=["S1", "S2"])
def test_generate_beams_with_processors(dtype, kw):
    ref, ours = _model(dtype)
    pix = _pix(NB, 64).to(DEV)
    what = f"beams K=3 {dtype} {kw}"
    out, gaps = _beam_replay(ours, pix, 3, 1, kw, what)
    _properties(out, kw, what)
    _against_transformers(out, _hf_generate(ref, 3, 1, kw), gaps, 1, what)
    eager = ours.generate(pix, _prompt(), max_new_tokens=MAX_NEW, num_beams=3, graph=False, **kw).cpu()
    assert torch.equal(out, eager), "graph replay must equal graph=False"


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("kw", [{}, S1], ids=["plain", "S1"])
def test_generate_returns_the_n_best_beams(dtype, n, kw):
    ref, ours = _model(dtype)
    pix = _pix(NB, 64).to(DEV)
    what = f"n-best K=3 n={n} {dtype} {kw}"
    out, gaps = _beam_replay(ours, pix, 3, n, kw, what)
    assert out.shape[0] == NB * n
    one = ours.generate(pix, _prompt(), max_new_tokens=MAX_NEW, num_beams=3, **kw).cpu()
    best = out.view(NB, n, -1)[:, 0]
    m = one.shape[1]
    assert m <= best.shape[1] and torch.equal(best[:, :m], one) and (best[:, m:] == FILL).all(), "rank 0 is the n = 1 result"
    _properties(out, kw, what)
    _against_transformers(out, _hf_generate(ref, 3, n, kw), gaps, n, what)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_generate_processors_change_the_captions_and_the_graph_follows(dtype):
    """the plain captions of this model repeat a bigram and end before eight new tokens somewhere, so the processors show; a call
    with other settings on the same captioner is not served by the captured step of the call before; neutral keywords are no
    keywords"""
    _, ours = _model(dtype, SHOW_SEED)
    pix = _pix(NB, 64).to(DEV)
    P = len(PROMPT) - 1
    plain = ours.generate(pix, _prompt(), max_new_tokens=MAX_NEW).cpu()
    caps = [_caption(r, P) for r in plain]
    assert any(repeated_ngrams(c, 2) for c in caps), caps
    assert any(EOS in c[P:] and len(c) - 1 - P < 8 for c in caps), caps
    with_s1 = ours.generate(pix, _prompt(), max_new_tokens=MAX_NEW, **S1).cpu()            # re-captures: other settings
    _properties(with_s1, S1, f"S1 after plain {dtype}")
    with_s2 = ours.generate(pix, _prompt(), max_new_tokens=MAX_NEW, **S2).cpu()
    _properties(with_s2, S2, f"S2 after S1 {dtype}")
    assert not torch.equal(with_s1[:, :P + 8], with_s2[:, :P + 8])
    again = ours.generate(pix, _prompt(), max_new_tokens=MAX_NEW).cpu()
    neutral = ours.generate(pix, _prompt(), max_new_tokens=MAX_NEW, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0,
                            min_new_tokens=0, num_return_sequences=1).cpu()
    assert torch.equal(plain, again) and torch.equal(plain, neutral)
    for kw in (S1, S2):
        for K in (1, 3):
            a = ours.generate(pix, _prompt(), max_new_tokens=MAX_NEW, num_beams=K, **kw).cpu()
            b = ours.generate(pix, _prompt(), max_new_tokens=MAX_NEW, num_beams=K, graph=False, **kw).cpu()
            assert torch.equal(a, b), (kw, K)
