"""GPU checks of sampled captioning: mh_sample_step against the restatement of tests/sampling_restatement.py (pinned on the CPU by
test_blip_sampling.py against transformers' own warpers), and BlipCaptioner.generate(do_sample=True) step by step against
transformers' processors and warpers on the traced logits.

What a draw is checked against: its uniform is the restated hash exactly; its token lies in the restated kept set; and the uniform lies
in the token's share [lo, hi) of the kept mass, widened by D = 2^-15 on both sides (twice the kernel's stated summation bound of
2^-16; it also covers expf and the x - max subtraction).  Every draw is checked, none is left out.  Inputs are picked so that no
kept / dropped decision of top-p hangs on rounding (sampling_restatement.top_p_margin >= D, asserted).

Token-for-token parity with BlipForConditionalGeneration.generate(do_sample=True) is not asked for and cannot be: torch.multinomial's
stream is not reproducible outside torch, and the kernel draws from a counter hash of (seed, row, column)."""
import numpy as np
import pytest
import torch

transformers = pytest.importorskip("transformers")

from logits_process_restatement import hf_processors, settings  # noqa: E402
from multimodal_propaganda_meme_classification_amd import ops  # noqa: E402
from sampling_restatement import (D, check_draw, draw_interval, hf_warpers, kept_set, sampling, tempered, top_p_margin,  # noqa: E402
                                  uniform)
from test_blip_caption import tiny_config  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EOS, PAD, BOS = 102, 0, 150
V, VP = 200, 256
P0, CAP = 3, 12
HIST0 = [BOS, 7, 8, 40]


# ---- 1. mh_sample_step against the restatement -------------------------------------------------------------------------------------------

def _sample_kernel(hist, logits, P, cap, proc, samp, seed, Vp=VP, finished=None, state2=0):
    """one step after the history hist int64 [B, col] on f32 logits [B, V']: (tokens, finished, state words, u, out_ids)"""
    B, col = hist.shape
    Vv = logits.shape[1]
    full = torch.full((B, Vp), 1e30)                     # a padded column would dominate every draw if it were read
    full[:, :Vv] = logits
    out = torch.full((B, cap), PAD, dtype=torch.int64)
    out[:, :col] = hist
    out = out.to(DEV)
    nxt = torch.zeros(B, dtype=torch.int64, device=DEV)
    fin = (torch.zeros(B, dtype=torch.int32) if finished is None else torch.tensor(finished, dtype=torch.int32)).to(DEV)
    st = torch.tensor([col - 1, 0, state2, 0], dtype=torch.int32, device=DEV)
    u = torch.full((B,), -1.0, device=DEV)
    ops.sample_step(full.to(DEV), Vv, out, nxt, fin, st, P, EOS, PAD, ops.sampling(**samp), ops.sample_rng(seed, DEV), u_out=u,
                    process=ops.logits_process(**proc))
    return nxt.cpu(), fin.cpu(), st.cpu().tolist(), u.cpu(), out.cpu()


def _check(what, hist, logits, P, cap, proc, samp, seed, Vp=VP):
    """the restated uniform exactly; the token in the restated kept set and u in its interval +- D; the bookkeeping of the step"""
    proc, samp = settings(**proc), sampling(**samp)
    B, col = hist.shape
    margin = top_p_margin(logits, hist, P, EOS, proc, samp)
    assert margin >= D, (what, "precondition: a top-p decision within 2^-15 of its boundary", margin)
    kept = kept_set(logits, hist, P, EOS, proc, samp)
    lo, hi = draw_interval(logits, hist, P, EOS, proc, samp)
    tok, fin, state, u, out = _sample_kernel(hist, logits, P, cap, proc, samp, seed, Vp)
    want_u = [uniform(seed, r, col) for r in range(B)]
    assert u.tolist() == want_u, (what, u.tolist(), want_u)
    check_draw(what, tok, want_u, kept, lo, hi)
    assert torch.equal(out[:, col], tok) and torch.equal(out[:, :col], hist) and (out[:, col + 1:] == PAD).all(), what
    assert fin.tolist() == [int(t == EOS) for t in tok.tolist()], what
    assert state == [col, 0, sum(fin.tolist()), col + 1 if all(fin.tolist()) else 0], (what, state)
    return tok, want_u, kept


def _hist(B, g, row0=HIST0):
    h = torch.randint(1, 7, (B, len(row0)), generator=g)      # few tokens: the other rows' n-grams repeat too
    h[0] = torch.tensor(row0)
    h[:, 0] = BOS
    return h


def _logits(B, g, over=None, Vv=V):
    x = 5 * torch.rand(B, Vv, generator=g) - 2.5               # no ties
    for t, v in (over or {}).items():
        x[0, t] = v
    return x


# name: (history of row 0, {token: logit} of row 0, processor settings, sampling settings)
CASES = {
    "temperature 0.7": (HIST0, {}, {}, dict(temperature=0.7)),
    "temperature 1": (HIST0, {}, {}, {}),
    "temperature 1.5": (HIST0, {}, {}, dict(temperature=1.5)),
    "top_k 1": (HIST0, {}, {}, dict(top_k=1)),
    "top_k 5": (HIST0, {}, {}, dict(top_k=5)),
    "top_k V": (HIST0, {}, {}, dict(top_k=V)),
    "top_k V + 10": (HIST0, {}, {}, dict(top_k=V + 10)),
    "top_p 0.9": (HIST0, {}, {}, dict(top_p=0.9)),
    "top_p 0.5": (HIST0, {}, {}, dict(top_p=0.5)),
    "top_p 1e-6": (HIST0, {}, {}, dict(top_p=1e-6)),
    "top-k and top-p": (HIST0, {}, {}, dict(temperature=1.3, top_k=20, top_p=0.8)),
    "all three, sharp": (HIST0, {}, {}, dict(temperature=0.7, top_k=50, top_p=0.9)),
    "repetition penalty": (HIST0, {40: 6.0, 41: 5.5}, dict(repetition_penalty=1.5), dict(top_k=1)),
    "n-gram ban": ([BOS, 7, 8, 20, 21, 20], {21: 9.0}, dict(no_repeat_ngram_size=2), dict(top_p=0.9)),
    "min_length": (HIST0, {EOS: 9.0}, dict(min_length=6), dict(top_k=5)),
    "min_new_tokens": (HIST0, {EOS: 9.0}, dict(min_new_tokens=3), dict(temperature=0.7, top_k=10)),
    "every processor": ([BOS, 7, 8, 20, 21, 20], {21: 9.0, EOS: 8.0, 20: 7.0}, dict(repetition_penalty=1.2, no_repeat_ngram_size=2,
                                                                                   min_length=8, min_new_tokens=4),
                        dict(temperature=1.3, top_k=20, top_p=0.8)),
    "a tie at the top-k threshold": (HIST0, {40: 9.0, 41: 8.0, 42: 7.0, 43: 7.0}, {}, dict(top_k=3)),
    "a tie straddling the top-p boundary": (HIST0, {60: 12.0, 61: 11.0, 62: 11.0}, {}, dict(top_p=0.75)),
}
TIES = ("a tie at the top-k threshold", "a tie straddling the top-p boundary")


def case_inputs(name, B):
    row0, over, proc, samp = CASES[name]
    g = torch.Generator().manual_seed(1000 * B + sorted(CASES).index(name))
    return _hist(B, g, row0), _logits(B, g, over), settings(**proc), sampling(**samp)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_sample_step(name, B):
    hist, logits, proc, samp = case_inputs(name, B)
    for seed in (11, 2 ** 40 + 5):
        tok, _, kept = _check(name, hist, logits, P0, CAP, proc, samp, seed)
    n0 = int(kept[0].sum())
    if name.startswith("top_k 1") or name == "top_p 1e-6":
        assert n0 == 1 and int(tok[0]) == int(logits[0].argmax())
    if name == "top_k 5":
        assert (kept.sum(1) == 5).all()
    if name in ("top_k V", "top_k V + 10", "temperature 1"):
        assert (kept.sum(1) == V).all()
    if name == "repetition penalty":
        assert int(tok[0]) == 41                                  # 6.0 / 1.5 falls behind 5.5
    if name in ("n-gram ban", "every processor"):
        assert not kept[0, 21] and int(logits[0].argmax()) == 21       # the row's best token is banned, and never drawn
    if name in ("min_length", "min_new_tokens", "every processor"):
        assert not kept[:, EOS].any()
    if name == "a tie at the top-k threshold":
        assert kept[0].nonzero().flatten().tolist() == [40, 41, 42, 43]          # top_k = 3 keeps four: both of the tie
    if name == "a tie straddling the top-p boundary":
        # masses 0.571 | 0.210, 0.210 | ...: 0.75 is reached inside the pair of equal values, and both are kept
        assert kept[0].nonzero().flatten().tolist() == [60, 61, 62]


def test_uniforms_differ_between_rows_columns_and_seeds():
    g = torch.Generator().manual_seed(3)
    seen = {}
    for seed in (11, 12, 2 ** 63 + 11):                            # (the last differs from 11 in the high word only)
        for col in (4, 5, 9):
            hist = _hist(3, g, HIST0 + [9] * (col - 4))
            _, _, _, u, _ = _sample_kernel(hist, _logits(3, g), P0, CAP, settings(), sampling(), seed)
            for r in range(3):
                assert float(u[r]) == uniform(seed, r, col)
                seen[(seed, r, col)] = float(u[r])
    assert len(set(seen.values())) == len(seen) == 27


def _hash32_np(x):
    M = np.uint32
    x = x ^ (x >> M(16))
    x = x * M(0x7feb352d)
    x = x ^ (x >> M(15))
    x = x * M(0x846ca68b)
    return x ^ (x >> M(16))


def test_u_next_to_one_draws_the_last_kept_index():
    """the largest uniform there is, 1 - 2^-24, found by searching a million seeds with the restated hash: u * Z is then Z itself or
    one ulp below it, and the draw is the last kept index in index order -- by the prefix rule, or, where rounding leaves no prefix
    above the target, by the rule that takes its place; never an unkept index, never the greedy token"""
    lo = np.arange(9_000_000, 10_000_000, dtype=np.uint32)
    h = _hash32_np(lo ^ np.uint32(0x9E3779B9))
    for add in (0, 0, 4):                                          # seed_hi, row, column
        h = _hash32_np(h + np.uint32(add))
    seeds = lo[(h >> np.uint32(8)) == np.uint32(0xFFFFFF)].tolist()
    assert seeds and all(uniform(s, 0, 4) == 1 - 2.0 ** -24 for s in seeds)
    for B in (1, 3):
        g = torch.Generator().manual_seed(50 + B)
        hist, logits = _hist(B, g), _logits(B, g, {5: 4.0, 90: 3.0, 190: 3.5})
        for samp in (dict(top_k=3), dict(top_k=3, top_p=0.99), {}):
            tok, _, kept = _check(f"u near 1 {samp}", hist, logits, P0, CAP, {}, samp, seeds[0])
            last = int(kept[0].nonzero().max())
            assert int(tok[0]) == last != int(logits[0].argmax()), (samp, tok.tolist(), last)
        assert last == V - 1


def test_top_k_one_is_greedy_whatever_u_is():
    g = torch.Generator().manual_seed(7)
    hist, logits = _hist(3, g), _logits(3, g)
    full = torch.full((3, VP), 1e30)
    full[:, :V] = logits
    out = torch.full((3, CAP), PAD, dtype=torch.int64)
    out[:, :4] = hist
    nxt, fin = torch.zeros(3, dtype=torch.int64, device=DEV), torch.zeros(3, dtype=torch.int32, device=DEV)
    ops.greedy_step(full.to(DEV), V, out.to(DEV), nxt, fin, torch.tensor([3, 0, 0, 0], dtype=torch.int32, device=DEV), P0, EOS, PAD)
    us = set()
    for seed in range(20, 28):
        for T in (0.7, 1.0, 1.5):
            tok, _, _, u, _ = _sample_kernel(hist, logits, P0, CAP, settings(), sampling(top_k=1, temperature=T), seed)
            assert torch.equal(tok, nxt.cpu()), (seed, T)
            us |= set(u.tolist())
    assert len(us) == 24 and max(us) > 0.9 and min(us) < 0.1


def test_prompt_column_finished_row_eos_and_state():
    g = torch.Generator().manual_seed(8)
    hist, logits = _hist(3, g), _logits(3, g)
    samp = sampling(top_k=1)
    # inside the prompt (prompt_len 6 > column 4): the prompt's own next token, read from out_ids; nothing finishes
    B, col = hist.shape
    full = torch.full((B, VP), 1e30)
    full[:, :V] = logits
    out = torch.full((B, CAP), PAD, dtype=torch.int64)
    out[:, :col] = hist
    out[:, col] = torch.tensor([11, EOS, 13])                      # (an eos inside the prompt finishes nothing)
    out = out.to(DEV)
    nxt, fin = torch.zeros(B, dtype=torch.int64, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
    st = torch.tensor([col - 1, 0, 0, 0], dtype=torch.int32, device=DEV)
    u = torch.zeros(B, device=DEV)
    ops.sample_step(full.to(DEV), V, out, nxt, fin, st, 6, EOS, PAD, ops.sampling(**samp), ops.sample_rng(1, DEV), u_out=u)
    assert nxt.tolist() == [11, EOS, 13] and fin.tolist() == [0, 0, 0] and st.tolist() == [col, 0, 0, 0]
    assert u.tolist() == [uniform(1, r, col) for r in range(B)]
    # row 0 draws eos and finishes, row 1 had finished before (pad), row 2 goes on
    logits[0, EOS] = 50.0
    tok, fin, state, _, _ = _sample_kernel(hist, logits, P0, CAP, settings(), samp, 1, finished=[0, 1, 0], state2=1)
    assert tok.tolist() == [EOS, PAD, int(logits[2].argmax())] and fin.tolist() == [1, 1, 0] and state == [col, 0, 2, 0]
    # the last row finishes: the output length appears
    logits[2, EOS] = 50.0
    tok, fin, state, _, _ = _sample_kernel(hist, logits, P0, CAP, settings(), samp, 1, finished=[0, 1, 0], state2=1)
    assert tok.tolist() == [EOS, PAD, EOS] and fin.tolist() == [1, 1, 1] and state == [col, 0, 3, col + 1]


@pytest.mark.parametrize("samp", [dict(top_p=0.9), dict(temperature=0.7, top_k=50, top_p=0.9), dict(temperature=1.5), dict(top_k=3)],
                         ids=["top_p", "all", "whole-row", "top_k"])
def test_blip_vocabulary(samp):
    """one row of the BLIP vocabulary, the only size where a wave walks many trips: thirty peaks over a flat tail of 30494 tokens that
    holds about 1 % of the mass, so the top-p boundary falls between two peaks; with a processor on, so the bitmaps' last words are read"""
    Vv, Vp = 30524, 30528
    g = torch.Generator().manual_seed(9)
    x = 5 * torch.rand(1, Vv, generator=g) - 2.5
    peaks = torch.randperm(Vv, generator=g)[:30]
    x[0, peaks] = 14.0 - 0.2 * torch.arange(30.0) + 0.05 * torch.rand(30, generator=g)
    x[0, Vv - 1], x[0, 0] = 13.1, 12.9                            # the row's two ends are peaks too
    hist = torch.tensor([[30522, 5, 6, int(peaks[0])]])
    for seed in (1, 2, 3):
        _check(f"V=30524 {samp}", hist, x, P0, CAP, dict(repetition_penalty=1.3), samp, seed, Vp=Vp)


def test_distribution_chi_square():
    """16384 rows with the same 16 logits in one launch, top_k = 8, temperature 1.3: no row draws an unkept token, and Pearson's
    chi-square of the counts against the float64 probabilities stays below the 1 - 1e-9 quantile of chi2(7) -- the seed is fixed, so
    the result is deterministic; an off-by-one interval or a wrong Z gives thousands"""
    from scipy.stats import chi2
    B, Vv = 16384, 16
    row = torch.tensor([2.0, -3.0, 1.7, -2.5, 1.4, -3.5, 1.1, -4.0, 0.8, -2.8, 0.5, -3.2, 0.2, -2.2, -0.1, -5.0])
    samp = sampling(top_k=8, temperature=1.3)
    hist = torch.tensor([[BOS, 7, 8, 9]])
    kept = kept_set(row[None], hist, P0, EOS, settings(), samp)[0]
    lo, hi = draw_interval(row[None], hist, P0, EOS, settings(), samp)
    p = (hi - lo)[0][kept]
    assert int(kept.sum()) == 8 and float(p.min()) >= 1 / 256 and abs(float(p.sum()) - 1) < 1e-12
    tok, fin, state, u, _ = _sample_kernel(hist.repeat(B, 1), row[None].repeat(B, 1), P0, CAP, settings(), samp, 20240229, Vp=16)
    assert kept[tok].all(), "a row drew an unkept token"
    counts = torch.bincount(tok, minlength=Vv)[kept].double()
    stat = float(((counts - B * p) ** 2 / (B * p)).sum())
    bound = float(chi2.ppf(1 - 1e-9, 7))
    print(f"chi-square {stat:.3f} (bound {bound:.3f}), counts {counts.tolist()}")
    assert stat < bound, (stat, bound, counts.tolist())
    assert state[:3] == [4, 0, 0] and not fin.any() and 0.49 < float(u.mean()) < 0.51


def test_deterministic_and_the_graph_replay_is_the_eager_run():
    g = torch.Generator().manual_seed(10)
    B = 3
    hist, logits = _hist(B, g), _logits(B, g)
    samp, proc = sampling(temperature=1.3, top_k=20, top_p=0.8), settings(repetition_penalty=1.2)
    a = _sample_kernel(hist, logits, P0, CAP, proc, samp, 77)
    b = _sample_kernel(hist, logits, P0, CAP, proc, samp, 77)
    assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3])
    full = torch.full((B, VP), 1e30)
    full[:, :V] = logits
    full = full.to(DEV)
    out0 = torch.full((B, CAP), PAD, dtype=torch.int64)
    out0[:, :4] = hist
    out = out0.to(DEV)
    nxt, fin = torch.zeros(B, dtype=torch.int64, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
    st = torch.tensor([3, 0, 0, 0], dtype=torch.int32, device=DEV)
    u = torch.zeros(B, device=DEV)
    rng, s, p = ops.sample_rng(77, DEV), ops.sampling(**samp), ops.logits_process(**proc)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.sample_step(full, V, out, nxt, fin, st, P0, EOS, PAD, s, rng, u_out=u, process=p)
    for seed in (77, 78):                                          # the captured launch reads the seed from the device
        ops.set_sample_rng(rng, seed)
        out.copy_(out0), fin.zero_(), st.copy_(torch.tensor([3, 0, 0, 0], dtype=torch.int32))
        graph.replay()
        want = _sample_kernel(hist, logits, P0, CAP, proc, samp, seed)
        assert torch.equal(nxt.cpu(), want[0]) and torch.equal(u.cpu(), want[3]) and st.tolist() == want[2], seed


def test_sample_step_refusals():
    g = torch.Generator().manual_seed(6)
    x = torch.rand(1, 40000, generator=g).to(DEV)
    out = torch.zeros(1, 8, dtype=torch.int64, device=DEV)
    nxt, fin = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    st = torch.zeros(4, dtype=torch.int32, device=DEV)
    rng = ops.sample_rng(1, DEV)
    with pytest.raises(ValueError):                                # V above MH_PROCESS_MAX_VOCAB, processors or not
        ops.sample_step(x, 40000, out, nxt, fin, st, 1, EOS, PAD, ops.sampling(), rng)
    assert st.tolist() == [0, 0, 0, 0]
    with pytest.raises(TypeError):
        ops.sample_step(x, 30000, out, nxt, fin, st, 1, EOS, PAD, dict(top_k=3), rng)
    with pytest.raises(TypeError):
        ops.sample_step(x, 30000, out, nxt, fin, st, 1, EOS, PAD, ops.sampling(), torch.zeros(4, device=DEV))
    ops.sample_step(x, 30000, out, nxt, fin, st, 1, EOS, PAD, ops.sampling(), rng)
    assert st.tolist()[0] == 1 and 0 <= int(nxt[0]) < 30000


# ---- 2. BlipCaptioner.generate(do_sample=True) --------------------------------------------------------------------------------------

from test_blip_caption_gpu import _pair, _pix  # noqa: E402

PROMPT = [101, 7, 8, 9, 102]
NB, MAX_NEW = 3, 12
_models = {}
_ambiguous = {"steps": 0, "ambiguous": 0}


def _model(dtype="fp16"):
    if dtype not in _models:
        _models[dtype] = _pair(tiny_config(), dtype, seed=17, eos_boost=1.0)[1]
    return _models[dtype]


def _prompt(B=NB):
    return torch.tensor([PROMPT] * B)


def _sampled_replay(ours, pix, kw, seed, n=1, what=""):
    """generate with the trace hook; then, per step and row: the traced uniform is the restated hash, the traced token lies in the kept
    set that transformers' own processors and warpers give for the traced logits and history, and u lies in the token's interval +- D.
    A step whose top-p boundary has a token within D of it may match the restated set instead; such steps are counted."""
    B = pix.shape[0]
    R = B * n
    proc = {k: v for k, v in kw.items() if k in settings()}
    samp = dict(dict(top_k=50), **{k: v for k, v in kw.items() if k in sampling()})          # generate's default top_k is 50
    trace = []
    out = ours.generate(pix, _prompt(B), max_new_tokens=MAX_NEW, poll_every=1, do_sample=True, seed=seed, num_return_sequences=n,
                        _trace=trace, **kw).cpu()
    P = len(PROMPT) - 1
    ids = _prompt(B)
    ids[:, 0] = ours.text_cfg["bos_token_id"]
    hist = ids[:, :P].repeat_interleave(n, 0)
    hf = lambda h, x: hf_warpers(samp)(h, hf_processors(P, EOS, proc)(h, x))
    fin = torch.zeros(R, dtype=torch.bool)
    for i, tr in enumerate(trace):
        col = i + 1
        chosen = tr["next_ids"].cpu()
        assert tr["u"].cpu().tolist() == [uniform(seed, r, col) for r in range(R)], (what, col)
        if col < P:
            assert torch.equal(chosen, ids[:, col].repeat_interleave(n, 0)), (what, col)
            continue
        logits = tr["logits"].cpu().float()
        assert logits.shape == (R, ours.text_cfg["vocab_size"])
        hf_kept = hf(hist, logits.clone()) > float("-inf")
        kept = kept_set(logits, hist, P, EOS, proc, samp)
        lo, hi = draw_interval(logits, hist, P, EOS, proc, samp)
        for r in range(R):
            if fin[r]:
                assert int(chosen[r]) == PAD, (what, col, r)
                continue
            t = int(chosen[r])
            _ambiguous["steps"] += 1
            if top_p_margin(logits[r:r + 1], hist[r:r + 1], P, EOS, proc, samp) < D:
                _ambiguous["ambiguous"] += 1
                assert hf_kept[r, t] or kept[r, t], (what, col, r, t)
            else:
                assert torch.equal(hf_kept[r], kept[r]), (what, col, r, "the restatement left transformers' kept set")
                assert hf_kept[r, t], (what, col, r, t)
            if kept[r, t]:
                u = uniform(seed, r, col)
                assert float(lo[r, t]) - D <= u < float(hi[r, t]) + D, (what, col, r, t, u, float(lo[r, t]), float(hi[r, t]))
        assert tr["finished"].cpu().bool().tolist() == (fin | (chosen == EOS)).tolist(), (what, col)
        hist = torch.cat([hist, chosen[:, None]], 1)
        fin |= chosen == EOS
    assert torch.equal(out, hist[:, :out.shape[1]]), what
    assert _ambiguous["ambiguous"] * 10 <= _ambiguous["steps"], _ambiguous
    return out


GEN_CASES = [dict(), dict(top_k=0, top_p=0.9), dict(temperature=0.7, top_k=20, top_p=0.8),
             dict(temperature=1.5, top_k=0, repetition_penalty=1.2, no_repeat_ngram_size=2, min_new_tokens=6)]


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("kw", GEN_CASES, ids=["defaults", "top_p", "all", "processors"])
def test_generate_sampled_steps_follow_transformers_warpers(dtype, kw):
    ours = _model(dtype)
    pix = _pix(NB, 64).to(DEV)
    out = _sampled_replay(ours, pix, kw, 1234, what=f"{dtype} {kw}")
    eager = ours.generate(pix, _prompt(), max_new_tokens=MAX_NEW, do_sample=True, seed=1234, graph=False, **kw).cpu()
    assert torch.equal(out, eager), "graph replay must equal graph=False"
    if kw.get("min_new_tokens"):
        assert not (out[:, 4:4 + kw["min_new_tokens"]] == EOS).any()


def test_generate_seeds():
    ours = _model()
    pix = _pix(NB, 64).to(DEV)
    kw = dict(max_new_tokens=MAX_NEW, do_sample=True, top_k=0, temperature=1.5)
    a = ours.generate(pix, _prompt(), seed=5, **kw).cpu()
    b = ours.generate(pix, _prompt(), seed=5, **kw).cpu()
    c = ours.generate(pix, _prompt(), seed=6, **kw).cpu()
    assert torch.equal(a, b), "the same seed gives the same captions"
    assert a.shape != c.shape or not torch.equal(a, c), "another seed gives other captions (served by the same captured step)"
    torch.manual_seed(7)
    d = ours.generate(pix, _prompt(), **kw).cpu()
    torch.manual_seed(7)
    e = ours.generate(pix, _prompt(), **kw).cpu()
    f = ours.generate(pix, _prompt(), **kw).cpu()                   # the generator has moved on
    assert torch.equal(d, e) and (d.shape != f.shape or not torch.equal(d, f))


def test_generate_top_k_one_is_the_greedy_caption():
    ours = _model()
    pix = _pix(NB, 64).to(DEV)
    greedy = ours.generate(pix, _prompt(), max_new_tokens=MAX_NEW).cpu()
    for seed in (1, 2):
        got = ours.generate(pix, _prompt(), max_new_tokens=MAX_NEW, do_sample=True, top_k=1, temperature=0.7, seed=seed).cpu()
        assert torch.equal(got, greedy), seed


def test_generate_num_return_sequences():
    """three captions per image as [9, L] rows [image][k]: they share the prompt and differ.  They equal three single calls in shape
    only: the hash is keyed by the row, image * 3 + k here and image there, so the draws differ -- nothing to assert."""
    ours = _model()
    pix = _pix(NB, 64).to(DEV)
    kw = dict(temperature=1.5, top_k=0)
    out = _sampled_replay(ours, pix, kw, 99, n=3, what="n=3")
    assert out.shape[0] == 9
    P = len(PROMPT) - 1
    rows = out.view(NB, 3, -1)
    assert (rows[:, :, 1:P] == torch.tensor(PROMPT[1:P])).all() and (rows[:, :, 0] == BOS).all()
    for b in range(NB):
        assert len({tuple(r.tolist()) for r in rows[b]}) == 3, f"the three captions of image {b} must differ"
    # the three rows of an image attend to that image (one copy of its cross-attention k / v): with top_k = 1 they are its greedy caption
    greedy = ours.generate(pix, _prompt(), max_new_tokens=MAX_NEW).cpu()
    thrice = ours.generate(pix, _prompt(), max_new_tokens=MAX_NEW, do_sample=True, top_k=1, seed=99, num_return_sequences=3).cpu()
    assert torch.equal(thrice, greedy.repeat_interleave(3, 0))


def test_greedy_and_beams_are_untouched_by_sampled_calls():
    """the history rule of test_history_independence_gpu.py: a call's result depends on its arguments, never on the calls before it"""
    ours = _model()
    pix = _pix(NB, 64).to(DEV)
    greedy = ours.generate(pix, _prompt(), max_new_tokens=MAX_NEW).cpu()
    beams = ours.generate(pix, _prompt(), max_new_tokens=MAX_NEW, num_beams=3).cpu()
    sampled = ours.generate(pix, _prompt(), max_new_tokens=MAX_NEW, do_sample=True, seed=3, temperature=1.5, top_k=0).cpu()
    ours.generate(pix, _prompt(), max_new_tokens=MAX_NEW, do_sample=True, seed=4, num_return_sequences=2, repetition_penalty=1.3)
    assert torch.equal(ours.generate(pix, _prompt(), max_new_tokens=MAX_NEW).cpu(), greedy)
    ours.generate(pix, _prompt(), max_new_tokens=MAX_NEW, do_sample=True, seed=4)
    assert torch.equal(ours.generate(pix, _prompt(), max_new_tokens=MAX_NEW, num_beams=3).cpu(), beams)
    assert torch.equal(ours.generate(pix, _prompt(), max_new_tokens=MAX_NEW, do_sample=True, seed=3, temperature=1.5, top_k=0).cpu(), sampled)


@pytest.mark.parametrize("kw", [dict(do_sample=True, num_beams=2), dict(num_return_sequences=2), dict(do_sample=True, temperature=0.0),
                                dict(do_sample=True, temperature=float("nan")), dict(do_sample=True, top_k=-1),
                                dict(do_sample=True, top_k=2.5), dict(do_sample=True, top_p=0.0), dict(do_sample=True, top_p=1.5),
                                dict(do_sample=True, seed=1.5), dict(do_sample=True, top_p="0.9"), dict(do_sample=1),
                                dict(do_sample=True, num_return_sequences=400)])
def test_generate_refusals_on_the_device(kw):
    ours = _model()
    pix = _pix(NB, 64).to(DEV)
    control = ours.generate(pix, _prompt(), max_new_tokens=2, do_sample=True, seed=1)      # a sampled call as such is accepted here
    assert control.shape[0] == NB
    with pytest.raises(ValueError):
        ours.generate(pix, _prompt(), max_new_tokens=MAX_NEW, **kw)
