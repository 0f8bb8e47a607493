"""The logits processors of the decode step, restated in torch for the processor tests (not a test module).

``process``            RepetitionPenalty, NoRepeatNGram, MinLength and MinNewTokensLength as include/memehip.h documents them, in that
                       order, on scores of any float dtype (float32 for the greedy kernel: one multiply or divide per value, so the
                       result is exact; float64 for the beam kernel).
``hf_processors``      transformers' own four processors in a ``LogitsProcessorList``, in ``_get_logits_processor``'s order.
``greedy_ref``         ``process`` on the raw logits, then the argmax (first maximum).
``beam_ref_step``      ``process`` on the row's log-softmax, composed with ``beam_restatement.ref_step``.
``beam_hf_step``       transformers' processors on transformers' log-softmax, composed with ``beam_restatement.hf_step``.

Settings travel as a dict ``dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, min_new_tokens=0)`` (missing keys are
neutral).  hist: int64 [R, L], the row's tokens so far, prompt included; P: the prompt length."""
import torch
from transformers import (LogitsProcessorList, MinLengthLogitsProcessor, MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor,
                          RepetitionPenaltyLogitsProcessor)

import beam_restatement

NEUTRAL = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, min_new_tokens=0)


def settings(**kw):
    unknown = set(kw) - set(NEUTRAL)
    assert not unknown, unknown
    return dict(NEUTRAL, **kw)


def banned_tokens(row, n):
    """the tokens NoRepeatNGram(n) bans after the sequence `row` (a list of ints)"""
    L = len(row)
    if n <= 0 or L < n:
        return set()
    tail = row[L - (n - 1):] if n > 1 else []
    return {row[j] for j in range(n - 1, L) if row[j - (n - 1):j] == tail}


def process(hist, scores, P, eos, s):
    """scores [R, V] -> processed copy, in scores.dtype"""
    s = settings(**s)
    R, V = scores.shape
    L = hist.shape[1]
    out = scores.clone()
    p = torch.tensor(s["repetition_penalty"], dtype=torch.float32).to(scores.dtype)      # the C ABI carries the penalty as a float
    for r in range(R):
        row = [int(t) for t in hist[r]]
        if s["repetition_penalty"] != 1.0:
            for t in sorted({t for t in row if 0 <= t < V}):           # once per distinct id
                out[r, t] = out[r, t] * p if out[r, t] < 0 else out[r, t] / p
        for t in banned_tokens(row, s["no_repeat_ngram_size"]):
            if 0 <= t < V:
                out[r, t] = float("-inf")
        if 0 <= eos < V and (L < s["min_length"] or (s["min_new_tokens"] > 0 and L - P < s["min_new_tokens"])):
            out[r, eos] = float("-inf")
    return out


def hf_processors(P, eos, s):
    s = settings(**s)
    procs = LogitsProcessorList()
    if s["repetition_penalty"] != 1.0:
        procs.append(RepetitionPenaltyLogitsProcessor(penalty=float(s["repetition_penalty"])))
    if s["no_repeat_ngram_size"] > 0:
        procs.append(NoRepeatNGramLogitsProcessor(s["no_repeat_ngram_size"]))
    if s["min_length"] > 0:
        procs.append(MinLengthLogitsProcessor(s["min_length"], eos))
    if s["min_new_tokens"] > 0:
        procs.append(MinNewTokensLengthLogitsProcessor(P, s["min_new_tokens"], eos))
    return procs


def greedy_ref(logits, hist, P, eos, s):
    """float32 logits [B, V] -> (tokens [B], processed scores)"""
    sc = process(hist, logits.float(), P, eos, s)
    return sc.argmax(-1), sc


def beam_ref_step(logits, S, col, P, cap, lp, es, eos, s):
    """beam_restatement.ref_step with the processors between the log-softmax and the running score.  ref_step takes logits and applies
    its own log-softmax, so it is handed the processed log-probabilities y together with run_scores + logsumexp(y): its log-softmax
    gives y - logsumexp(y), and adding the shifted score restores y + score (to float64 rounding, 1e-16 relative; the tests demand
    margins of 1e-3).  The shift is taken back out of nothing: every value ref_step returns derives from y + score."""
    dt = S["run_scores"].dtype
    B, K, V = logits.shape
    x = logits.to(dt)
    m = x.max(-1, keepdim=True)[0]
    logp = (x - m) - torch.log(torch.exp(x - m).sum(-1, keepdim=True))
    hist = S["run_seq"][:, :, :col].reshape(B * K, col)
    y = process(hist, logp.reshape(B * K, V), P, eos, s).reshape(B, K, V)
    shifted = dict(S)
    shifted["run_scores"] = S["run_scores"] + torch.logsumexp(y, -1)
    return beam_restatement.ref_step(y, shifted, col, P, cap, lp, es, eos)


def beam_hf_step(logits, S, col, P, cap, lp, es, eos, s):
    """beam_restatement.hf_step with transformers' processors applied where _beam_search applies them: to log_softmax's output, with
    the flattened running sequences.  hf_step calls torch.nn.functional.log_softmax itself; for the length of the call that name
    returns the processed log-probabilities."""
    B, K, V = logits.shape
    hist = S["run_seq"][:, :, :col].reshape(B * K, col)
    procs = hf_processors(P, eos, s)
    real = torch.nn.functional.log_softmax

    def processed_log_softmax(x, dim=-1):
        return procs(hist, real(x, dim=dim))

    torch.nn.functional.log_softmax = processed_log_softmax
    try:
        return beam_restatement.hf_step(logits, S, col, P, cap, lp, es, eos)
    finally:
        torch.nn.functional.log_softmax = real


def repeated_ngrams(row, n):
    """the n-grams that occur more than once in `row` (a list of ints)"""
    seen, twice = set(), set()
    for i in range(len(row) - n + 1):
        g = tuple(row[i:i + n])
        (twice if g in seen else seen).add(g)
    return twice
