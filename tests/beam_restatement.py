"""One beam-search step, restated in torch for the beam tests (not a test module).

``ref_step``  the step as include/memehip.h documents it, in the dtype of the scores it is given (float64 for the kernel tests), with
              the documented tie rule: larger value first, then the lower flat index ``beam * V + token`` / the lower position.
``hf_step``   the same step through transformers' own helpers (``GenerationMixin._get_top_k_continuations`` ...), called in the order
              ``_beam_search`` calls them, on float32 logits.

Both work on a dict of CPU tensors:
    run_scores [B, K], run_seq int64 [B, K, cap], fin_seq int64 [B, K, cap], fin_scores [B, K], fin_flags bool [B, K],
    fin_len int64 [B, K], heur bool [B]
and return (new state, tokens [B, K], parents [B, K], info).  A finished slot whose flag is off holds no beam: torch.topk may fill it
from any of the candidates that tie at -1e9, so ``same_finished`` compares sequences and lengths only where the flag is on.
"""
import torch
from transformers import GenerationMixin as GM

NEG = -1.0e9


def initial_state(prompt, K, cap, pad, dtype=torch.float32):
    """prompt int64 [B, P]"""
    B, P = prompt.shape
    seq = torch.full((B, K, cap), pad, dtype=torch.int64)
    seq[:, :, :P] = prompt[:, None, :]
    rs = torch.full((B, K), NEG, dtype=dtype)
    rs[:, 0] = 0.0
    return dict(run_scores=rs, run_seq=seq, fin_seq=seq.clone(), fin_scores=torch.full((B, K), NEG, dtype=dtype),
                fin_flags=torch.zeros(B, K, dtype=torch.bool), fin_len=torch.zeros(B, K, dtype=torch.int64),
                heur=torch.ones(B, dtype=torch.bool))


def _topk(vals, k):
    """values descending, ties to the lower position"""
    order = torch.sort(vals, dim=1, descending=True, stable=True)[1][:, :k]
    return torch.gather(vals, 1, order), order


def _take(t, idx):
    while idx.dim() < t.dim():
        idx = idx.unsqueeze(-1)
    return torch.take_along_dim(t, idx, 1)


def ref_step(logits, S, col, P, cap, lp, es, eos):
    """logits [B, K, V] (any float dtype); the arithmetic runs in S['run_scores'].dtype"""
    dt = S["run_scores"].dtype
    B, K, V = logits.shape
    N = 2 * K
    x = logits.to(dt)
    m = x.max(-1, keepdim=True)[0]
    logp = (x - m) - torch.log(torch.exp(x - m).sum(-1, keepdim=True))
    acc = (logp + S["run_scores"][:, :, None]).reshape(B, K * V)
    top, flat = _topk(acc, N)
    par, tok = flat // V, flat % V
    cand_seq = _take(S["run_seq"], par).clone()
    cand_seq[:, :, col] = tok
    hit = (tok == eos) | (col + 1 >= cap)
    rv = top + hit.to(dt) * NEG
    run_scores, sel = _topk(rv, K)
    new = dict(run_scores=run_scores, run_seq=_take(cand_seq, sel))
    tokens, parents = _take(tok, sel), _take(par, sel)
    did = hit & (torch.arange(N) < K)[None, :]
    pen = torch.tensor(float(col + 1 - P) ** lp, dtype=dt)
    fs = top / pen
    full = S["fin_flags"].all(1, keepdim=True) & (es is True)
    fs = fs + full.to(dt) * NEG
    fs = fs + (~S["heur"])[:, None].to(dt) * NEG
    fs = fs + (~did).to(dt) * NEG
    ms = torch.cat([S["fin_scores"], fs], 1)
    mseq = torch.cat([S["fin_seq"], cand_seq], 1)
    mflag = torch.cat([S["fin_flags"], did], 1)
    mlen = torch.cat([S["fin_len"], torch.full((B, N), col + 1 - P, dtype=torch.int64)], 1)
    new["fin_scores"], fsel = _topk(ms, K)
    new["fin_seq"], new["fin_flags"], new["fin_len"] = _take(mseq, fsel), _take(mflag, fsel), _take(mlen, fsel)
    hyp = (cap - P) if (es == "never" and lp > 0.0) else (col + 1 - P)
    best = run_scores[:, :1] / torch.tensor(float(hyp) ** lp, dtype=dt)
    worst = torch.where(new["fin_flags"], new["fin_scores"].min(1, keepdim=True)[0], torch.tensor(NEG, dtype=dt))
    new["heur"] = S["heur"] & (best > worst).any(1)
    closed = ~new["heur"] | (new["fin_flags"].all(1) & (es is True)) | hit.all(1)
    return new, tokens, parents, dict(top=top, closed=closed)


def hf_step(logits, S, col, P, cap, lp, es, eos):
    """float32 logits [B, K, V] through transformers' helpers, in _beam_search's order"""
    B, K, V = logits.shape
    N = 2 * K
    gen = cap - P
    rbi = torch.full((B, K, gen), -1, dtype=torch.int32)           # only the length of a finished beam is read from these
    log_probs = torch.nn.functional.log_softmax(logits.reshape(B * K, V).float(), dim=-1)
    log_probs = log_probs.reshape(B, K, V) + S["run_scores"][:, :, None]
    log_probs = log_probs.reshape(B, K * V)
    top, tseq, tbi = GM._get_top_k_continuations(GM, accumulated_log_probs=log_probs, running_sequences=S["run_seq"],
                                                 running_beam_indices=rbi, cur_len=col, decoder_prompt_len=P, do_sample=False,
                                                 beams_to_keep=N, num_beams=K, vocab_size=V, batch_size=B)
    hit = (tseq[:, :, col] == eos) | (col + 1 >= cap)
    run_seq, run_scores, run_bi = GM._get_running_beams_for_next_iteration(GM, topk_log_probs=top, topk_running_sequences=tseq,
                                                                          topk_running_beam_indices=tbi,
                                                                          next_token_hits_stopping_criteria=hit, num_beams=K)
    mask = torch.cat([torch.ones(K, dtype=torch.bool), torch.zeros(N - K, dtype=torch.bool)])
    # the finished beams' index rows: every generated position filled (0) up to the beam's length, -1 after it
    fin_bi = torch.where(torch.arange(gen)[None, None, :] < S["fin_len"][:, :, None], 0, -1).to(torch.int32)
    cand_bi = torch.where(torch.arange(gen)[None, None, :] <= col - P, 0, -1).to(torch.int32).expand(B, N, gen)
    fin_seq, fin_scores, fin_bi, fin_flags = GM._update_finished_beams(
        GM, sequences=S["fin_seq"], topk_running_sequences=tseq, beam_scores=S["fin_scores"], topk_log_probs=top, beam_indices=fin_bi,
        topk_running_beam_indices=cand_bi, is_early_stop_heuristic_unsatisfied=S["heur"][:, None], is_sent_finished=S["fin_flags"],
        next_token_hits_stopping_criteria=hit, top_num_beam_mask=mask, num_beams=K, cur_len=col, decoder_prompt_len=P,
        length_penalty=lp, early_stopping=es)
    heur = GM._check_early_stop_heuristic(is_early_stop_heuristic_unsatisfied=S["heur"][:, None], running_beam_scores=run_scores,
                                          beam_scores=fin_scores, is_sent_finished=fin_flags, cur_len=col + 1, max_length=cap,
                                          decoder_prompt_len=P, early_stopping=es, length_penalty=lp)
    new = dict(run_scores=run_scores, run_seq=run_seq, fin_seq=fin_seq, fin_scores=fin_scores, fin_flags=fin_flags,
               fin_len=((fin_bi + 1).bool()).sum(-1), heur=heur[:, 0])
    parents = run_bi[:, :, col - P].to(torch.int64) - (torch.arange(B) * K)[:, None]
    closed = ~new["heur"] | (fin_flags.all(1) & (es is True)) | hit.all(1)
    return new, run_seq[:, :, col], parents, dict(top=top, closed=closed)


def same_finished(a, b, tol):
    """flags equal; scores within tol where a beam is held and <= -1e8 on both sides elsewhere; sequences and lengths equal where held"""
    if not torch.equal(a["fin_flags"], b["fin_flags"]):
        return "flags"
    f = a["fin_flags"]
    if f.any() and float((a["fin_scores"][f].double() - b["fin_scores"][f].double()).abs().max()) > tol:
        return "scores"
    if (~f).any() and (float(a["fin_scores"][~f].max()) > -1e8 or float(b["fin_scores"][~f].max()) > -1e8):
        return "empty-slot scores"
    if not torch.equal(a["fin_seq"][f], b["fin_seq"][f]):
        return "sequences"
    if not torch.equal(a["fin_len"][f], b["fin_len"][f]):
        return "lengths"
    return None


def same_scores(a, b, tol):
    """running scores: within tol where real (> -1e8 in the reference b), <= -1e8 on both sides elsewhere"""
    real = b > -1e8
    ok = torch.equal(real, a > -1e8)
    if ok and real.any():
        ok = float((a[real].double() - b[real].double()).abs().max()) <= tol
    return ok
