"""GPU checks of beam-search captioning: mh_beam_step against a float64 restatement, mh_attn_decode_beams (kv_group, the cache's
ancestry table), and BlipCaptioner.generate(num_beams=K) against a replay through transformers' own helpers and against
BlipForConditionalGeneration.generate.  tests/beam_restatement.py holds the restatement (pinned on the CPU by test_blip_beam.py)."""
import pytest
import torch

transformers = pytest.importorskip("transformers")

from beam_restatement import hf_step, initial_state, ref_step, same_finished, same_scores  # noqa: E402
from conftest import parity_log  # noqa: E402
from multimodal_propaganda_meme_classification_amd import ops  # noqa: E402
from test_blip_caption import tiny_config  # noqa: E402
from test_blip_caption_gpu import _pair, _pix  # noqa: E402  (_pair randomises through _randomize)

pytestmark = pytest.mark.gpu
DEV = "cuda"
T16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
EOS, PAD = 102, 0
FILL = PAD or EOS   # what transformers' _beam_search pads its sequences with: a pad id of 0 counts as unset there, so eos
TOL = 1e-5          # f32 log-sum-exp over <= 30592 terms plus <= 140 additions, against float64
_SEQ = ("run_seq", "fin_seq")


# ---- 1. mh_beam_step against float64 -----------------------------------------------------------------------------------------

def _to_device(S, B, K, cap, col):
    """a beam_state holding the restatement's state S, about to consume position col - 1"""
    bs = ops.beam_state(B, K, cap, S["run_seq"][:, 0, :1], PAD, DEV)
    R = B * K
    for n in _SEQ:
        bs[n].copy_(S[n].reshape(R, cap).to(torch.int32))
    bs["run_scores"].copy_(S["run_scores"].reshape(R).float())
    bs["fin_scores"].copy_(S["fin_scores"].reshape(R).float())
    bs["fin_flags"].copy_(S["fin_flags"].reshape(R).to(torch.int32))
    bs["fin_len"].copy_(S["fin_len"].reshape(R).to(torch.int32))
    bs["heur"].copy_(S["heur"].to(torch.int32))
    bs["state"][0] = col - 1
    return bs


def _from_device(bs):
    B, K, cap = bs["B"], bs["K"], bs["cap"]
    c = lambda n: bs[n].cpu()
    return dict(run_scores=c("run_scores").view(B, K), run_seq=c("run_seq").view(B, K, cap).long(), fin_seq=c("fin_seq").view(B, K, cap).long(),
                fin_scores=c("fin_scores").view(B, K), fin_flags=c("fin_flags").view(B, K).bool(), fin_len=c("fin_len").view(B, K).long(),
                heur=c("heur").bool()), c("next_ids").view(B, K), c("parents").view(B, K).long(), c("state").tolist()


def _mid_state(B, K, cap, P, col, g, V, spread=0.5):
    """a search in progress at column col: distinct live beams with f32-representable scores, `spread` apart"""
    S = initial_state(torch.randint(1, 100, (B, P), generator=g), K, cap, PAD, torch.float64)
    S["run_seq"][:, :, P:col] = torch.randint(1, 100, (B, K, col - P), generator=g)
    S["run_scores"] = (-spread * torch.arange(K)[None, :] - torch.rand(B, K, generator=g)).float().double()
    return S


def _run_kernel_case(what, B, K, V, Vp, logits, S, col, P, cap, lp, es, tie=False):
    full = torch.full((B * K, Vp), 1e30)                       # the padded columns would win every selection if they were read
    full[:, :V] = logits.reshape(B * K, V)
    bs = _to_device(S, B, K, cap, col)
    ops.beam_step(full.to(DEV), V, bs, P, lp, es, EOS)
    got, tok, par, state = _from_device(bs)
    want, wtok, wpar, info = ref_step(logits.double(), S, col, P, cap, lp, es, EOS)
    gap = float((info["top"][:, :-1] - info["top"][:, 1:]).min())
    real = want["run_scores"] > -1e8
    err = float((got["run_scores"].double() - want["run_scores"])[real].abs().max()) if real.any() else 0.0
    parity_log(f"beam_step {what} B={B} K={K} V={V}: min float64 gap in the top 2K {gap:.3e}, max|running score err| {err:.3e}")
    ids_ok = torch.equal(tok, wtok) and torch.equal(par, wpar)
    if not ids_ok and not tie:
        print(f"id mismatch in a case without ties: float64 margin {gap:.3e}\n got {tok.tolist()} {par.tolist()}\nwant {wtok.tolist()} {wpar.tolist()}")
    assert ids_ok, what
    assert torch.equal(got["run_seq"], want["run_seq"]) and torch.equal(got["heur"], want["heur"]), what
    assert same_scores(got["run_scores"], want["run_scores"], TOL), what
    assert same_finished(got, want, TOL) is None, (what, same_finished(got, want, TOL))
    assert torch.equal(got["fin_seq"], want["fin_seq"]) and torch.equal(got["fin_len"], want["fin_len"]), what      # same tie rule: all slots
    assert state == [col, 0, 0, int(bool(info["closed"].all()))], (what, state)
    return got, want, info, tok, par


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K", [2, 3, 8])
def test_beam_step_first_step(B, K):
    """beams 1.. start at -1e9: every candidate comes from beam 0"""
    V, Vp, P, cap = 200, 256, 3, 10
    g = torch.Generator().manual_seed(10 * B + K)
    S = initial_state(torch.randint(1, 100, (B, P), generator=g), K, cap, PAD, torch.float64)
    logits = 3 * torch.randn(B, K, V, generator=g)
    _, _, _, _, par = _run_kernel_case("first step", B, K, V, Vp, logits, S, P, P, cap, 1.0, False)
    assert (par == 0).all()


def test_beam_step_large_vocabulary():
    B, K, V, Vp, P, cap = 3, 8, 30524, 30592, 3, 10
    g = torch.Generator().manual_seed(5)
    S = _mid_state(B, K, cap, P, 5, g, V)
    logits = 3 * torch.randn(B, K, V, generator=g)
    logits[:, 1, EOS] = 14.0
    _run_kernel_case("V=30524", B, K, V, Vp, logits, S, 5, P, cap, 1.0, False)


def _ranked(B, K, V, g, eos_rank):
    """logits whose top 2K candidates all come from beam 0 (with _mid_state(spread=20)), tokens 10.. in order, eos at rank eos_rank"""
    logits = torch.randn(B, K, V, generator=g).clamp(-3, 3)
    for j in range(2 * K):
        logits[:, 0, EOS if j == eos_rank else 10 + j] = 20.0 - j
    return logits


@pytest.mark.parametrize("where", ["inside", "outside"])
@pytest.mark.parametrize("BK", [(1, 2), (3, 3)])
def test_beam_step_eos_inside_and_outside_the_first_k(where, BK):
    B, K = BK
    V, Vp, P, cap, col = 200, 256, 3, 10, 5
    g = torch.Generator().manual_seed(20 + K)
    S = _mid_state(B, K, cap, P, col, g, V, spread=20.0)
    rank = 1 if where == "inside" else K
    got, _, _, tok, _ = _run_kernel_case(f"eos {where}", B, K, V, Vp, _ranked(B, K, V, g, rank), S, col, P, cap, 1.0, False)
    assert not (tok == EOS).any(), "eos never continues"
    assert got["fin_flags"][:, 0].all() == (where == "inside") and (got["fin_flags"].sum(1) == (1 if where == "inside" else 0)).all()
    if where == "inside":
        assert (got["fin_seq"][:, 0, col] == EOS).all() and (got["fin_len"][:, 0] == col + 1 - P).all()


def test_beam_step_exact_ties():
    """equal logits across beams (equal scores, identical rows) and within a beam: checked against the documented rule -- the lower
    flat index beam * V + token, then the lower position -- not against torch.topk"""
    B, K, V, Vp, P, cap, col = 1, 3, 200, 256, 3, 10, 5
    g = torch.Generator().manual_seed(31)
    S = _mid_state(B, K, cap, P, col, g, V)
    S["run_scores"][:] = -1.0
    row = torch.randn(V, generator=g).clamp(-3, 3)
    row[40] = row[7] = row[150] = 9.0                          # a three-way tie within the row
    logits = row[None, None, :].repeat(B, K, 1)                 # ... and the same row in every beam
    _, _, _, tok, par = _run_kernel_case("ties", B, K, V, Vp, logits, S, col, P, cap, 1.0, False, tie=True)
    assert tok.tolist() == [[7, 40, 150]] and par.tolist() == [[0, 0, 0]]      # 9 tied candidates: beam 0's three, by token


def test_beam_step_all_finished_with_early_stopping():
    B, K, V, Vp, P, cap, col = 3, 3, 200, 256, 3, 10, 6
    g = torch.Generator().manual_seed(41)
    S = _mid_state(B, K, cap, P, col, g, V, spread=20.0)
    S["fin_flags"][:] = True
    S["fin_scores"] = (-5.0 - torch.arange(K, dtype=torch.float64))[None, :].repeat(B, 1)
    S["fin_len"][:] = 2
    S["fin_seq"][:, :, P:P + 2] = torch.tensor([55, EOS])
    before = {n: S[n].clone() for n in ("fin_seq", "fin_scores", "fin_flags", "fin_len")}
    got, _, info, _, _ = _run_kernel_case("full + early_stopping", B, K, V, Vp, _ranked(B, K, V, g, 0), S, col, P, cap, 1.0, True)
    for n, v in before.items():                                 # a much better eos candidate arrives and is refused
        assert torch.equal(got[n].to(v.dtype), v), n
    assert info["closed"].all()
    # the same state without early stopping takes it
    got2, _, _, _, _ = _run_kernel_case("full, early_stopping False", B, K, V, Vp, _ranked(B, K, V, g, 0), S, col, P, cap, 1.0, False)
    assert (got2["fin_seq"][:, 0, col] == EOS).all()


@pytest.mark.parametrize("lp", [0.0, 1.0, 2.0])
@pytest.mark.parametrize("es", [False, "never"])
def test_beam_step_length_penalty(lp, es):
    B, K, V, Vp, P, cap, col = 3, 3, 200, 256, 3, 12, 7
    g = torch.Generator().manual_seed(51)
    S = _mid_state(B, K, cap, P, col, g, V, spread=20.0)
    S["fin_flags"][:, 0] = True                                 # one finished beam already: the new one is ranked against it
    S["fin_scores"][:, 0] = torch.tensor([-0.05, -0.6, -30.0], dtype=torch.float64)
    S["fin_len"][:, 0] = 2
    got, want, _, _, _ = _run_kernel_case(f"length_penalty {lp} {es}", B, K, V, Vp, _ranked(B, K, V, g, 0), S, col, P, cap, lp, es)
    assert ((want["fin_len"] == col + 1 - P).sum(1) == 1).all() and got["fin_flags"][:, :2].all()      # the new beam is in, ranked by score


def test_beam_step_last_step():
    """cur_len + 1 == max_length: every candidate stops, the first K finish, no image stays open"""
    B, K, V, Vp, P, cap = 3, 3, 200, 256, 3, 8
    g = torch.Generator().manual_seed(61)
    S = _mid_state(B, K, cap, P, cap - 1, g, V)
    got, _, info, _, _ = _run_kernel_case("last step", B, K, V, Vp, 3 * torch.randn(B, K, V, generator=g), S, cap - 1, P, cap, 1.0, False)
    assert got["fin_flags"].all() and info["closed"].all() and (got["run_scores"] <= -1e8).all()


def test_beam_step_done_image_keeps_its_finished_beams():
    B, K, V, Vp, P, cap, col = 3, 3, 200, 256, 3, 10, 6
    g = torch.Generator().manual_seed(71)
    S = _mid_state(B, K, cap, P, col, g, V, spread=20.0)
    S["heur"][1] = False                                        # image 1 is done
    S["fin_flags"][1] = True
    S["fin_scores"][1] = torch.tensor([-4.0, -5.0, -6.0], dtype=torch.float64)
    S["fin_len"][1] = 2
    S["fin_seq"][1, :, P:P + 2] = torch.tensor([66, EOS])
    got, _, info, _, _ = _run_kernel_case("done image", B, K, V, Vp, _ranked(B, K, V, g, 0), S, col, P, cap, 1.0, False)
    for n in ("fin_seq", "fin_scores", "fin_flags", "fin_len"):
        assert torch.equal(got[n][1].to(S[n].dtype), S[n][1]), n
    assert not got["heur"][1] and got["fin_flags"][0, 0] and got["fin_seq"][0, 0, col] == EOS      # the others moved
    assert info["closed"].tolist()[1] and not info["closed"].all()


def test_beam_step_inside_the_prompt_and_host_validation():
    B, K, V, P, cap = 2, 3, 200, 4, 9
    prompt = torch.tensor([[150, 7, 8, 9], [150, 17, 18, 19]])
    bs = ops.beam_state(B, K, cap, prompt, PAD, DEV)
    before = {n: v.clone() for n, v in bs.items() if isinstance(v, torch.Tensor)}
    logits = torch.randn(B * K, 256, device=DEV)
    ops.beam_step(logits, V, bs, P, 1.0, False, EOS)
    assert bs["next_ids"].view(B, K).tolist() == [[7] * K, [17] * K] and bs["parents"].view(B, K).tolist() == [[0, 1, 2]] * B
    assert bs["state"].tolist() == [1, 0, 0, 0]
    for n in ("run_scores", "run_seq", "fin_seq", "fin_scores", "fin_flags", "fin_len", "heur"):
        assert torch.equal(bs[n], before[n]), n
    with pytest.raises(Exception):
        ops.beam_step(logits[:, :6].contiguous(), 4, bs, P, 1.0, False, EOS)       # V < 2K
    with pytest.raises(ValueError):
        ops.beam_state(B, 9, cap, prompt, PAD, DEV)
    with pytest.raises(ValueError):
        ops.beam_step(logits, V, bs, P, 1.0, "always", EOS)


# ---- 2. kv_group ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("BKH", [(2, 3, 2), (4, 2, 12)])
@pytest.mark.parametrize("Ni", [17, 577])
def test_attn_decode_kv_group_is_the_repeated_call(dtype, BKH, Ni):
    B, K, H = BKH
    D, R = H * 64, B * K
    g = torch.Generator().manual_seed(Ni + H)
    q = torch.randn(R, D, generator=g).to(T16[dtype]).to(DEV)
    kv = (2 * torch.randn(B, Ni, 2 * D, generator=g)).to(T16[dtype]).to(DEV)
    rep = kv.repeat_interleave(K, 0).contiguous()
    out, want = (torch.full((R, D), float("nan"), dtype=T16[dtype], device=DEV) for _ in range(2))
    ns = ops.decode_splits(R, H, Ni)
    kf, rf = kv.view(-1), rep.view(-1)
    ops.attn_decode(q, kf, kf[D:], out, R, H, Ni, D, Ni * 2 * D, 2 * D, D, nsplit=ns, kv_group=K)
    ops.attn_decode(q, rf, rf[D:], want, R, H, Ni, D, Ni * 2 * D, 2 * D, D, nsplit=ns)
    assert torch.equal(out, want) and not torch.isnan(out.float()).any()
    with pytest.raises(ValueError):
        ops.attn_decode(q, kf, kf[D:], out, R, H, Ni, D, Ni * 2 * D, 2 * D, D, kv_group=R + 1)      # does not divide the rows


# ---- 3. the cache follows the beams --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_self_attention_cache_follows_the_beams(dtype):
    """four steps whose parents (set through the logits) include a beam chosen twice and a beam dropped: attention through the
    ancestry table is bit-identical to attention over an explicitly gathered cache, and each row writes slot t of itself only"""
    B, K, H, V, cap, P = 2, 3, 2, 200, 8, 1
    D, R = H * 64, B * K
    g = torch.Generator().manual_seed(3)
    bs = ops.beam_state(B, K, cap, torch.full((B, P), 150), PAD, DEV)
    cache = torch.zeros(R, cap, 2 * D, dtype=T16[dtype], device=DEV)
    logical = [[] for _ in range(R)]                            # per row: the k | v rows of its beam's positions 0..t-1
    wanted = [[0, 0, 2], [1, 1, 0], [2, 0, 1], [2, 2, 2]]
    for t, parents in enumerate(wanted):
        qkv = torch.randn(R, 3 * D, generator=g).to(T16[dtype]).to(DEV)
        before = cache.clone()
        out, ref_out = (torch.empty(R, D, dtype=T16[dtype], device=DEV) for _ in range(2))
        cf, qf = cache.view(-1), qkv.view(-1)
        ns = ops.decode_splits(R, H, cap)
        ops.attn_decode(qkv, cf, cf[D:], out, R, H, cap, 3 * D, cap * 2 * D, 2 * D, D, t_dev=bs["state"][0:1], kv_new=qf[D:], ld_new=3 * D,
                        nsplit=ns, src=bs["src"])
        gathered = torch.zeros_like(cache)
        for r in range(R):
            for j, row in enumerate(logical[r]):
                gathered[r, j] = row
        gf = gathered.view(-1)
        ops.attn_decode(qkv, gf, gf[D:], ref_out, R, H, cap, 3 * D, cap * 2 * D, 2 * D, D, t_dev=bs["state"][0:1], kv_new=qf[D:],
                        ld_new=3 * D, nsplit=ns)
        assert torch.equal(out, ref_out), t
        assert torch.equal(cache[:, t], qkv[:, D:]), t
        keep = torch.ones(cap, dtype=torch.bool)
        keep[t] = False
        assert torch.equal(cache[:, keep], before[:, keep]), t
        for r in range(R):
            logical[r] = logical[r] + [qkv[r, D:].clone()]
        # one beam step whose parents are `parents`: candidate k is (beam parents[k], token 10 + k)
        logits = torch.full((B, K, 256), -10.0)
        for k, p in enumerate(parents):
            logits[:, p, 10 + k] = 10.0
        bs["run_scores"].zero_()
        ops.beam_step(logits.view(R, 256).to(DEV), V, bs, P, 1.0, False, EOS)
        par = bs["parents"].view(B, K).cpu()
        assert sorted(par[0].tolist()) == sorted(parents) and torch.equal(par[0], par[1]), (t, par.tolist())
        logical = [logical[(r // K) * K + int(par[r // K, r % K])] for r in range(R)]
        assert int(bs["state"][0]) == t + 1
        src = bs["src"].cpu()
        assert ((src[:, :t + 1] // K) == torch.arange(R)[:, None] // K).all(), "a beam reads its own image's rows"


# ---- 4. replay through transformers' helpers -----------------------------------------------------------------------------------

SETTINGS = [(3, 1.0, False), (4, 2.0, True), (2, 0.0, False), (5, 1.0, "never")]
PROMPT = [101, 7, 8, 9, 102]
_models = {}


def _model(dtype, seed):
    if (dtype, seed) not in _models:
        _models[(dtype, seed)] = _pair(tiny_config(), dtype, seed=seed, eos_boost=1.0)
    return _models[(dtype, seed)]


def _replay(ours, pix, K, lp, es, max_new=12, what=""):
    """generate with the trace hook, then transformers' helpers on the recorded logits, step by step.  After each step the replay
    takes over the device's scores (they were just checked to TOL), so rounding differences do not pile up.  A running beam at
    -1e9 is dead (torch.topk takes it from candidates that tie in float32) and is not compared."""
    B = pix.shape[0]
    prompt = torch.tensor([PROMPT] * B)
    trace = []
    out = ours.generate(pix, prompt.clone(), max_new_tokens=max_new, num_beams=K, length_penalty=lp, early_stopping=es, poll_every=1,
                        _trace=trace).cpu()
    P, V = len(PROMPT) - 1, ours.text_cfg["vocab_size"]
    cap = P + max_new
    ids = prompt.clone()
    ids[:, 0] = ours.text_cfg["bos_token_id"]
    S = initial_state(ids[:, :P], K, cap, FILL)
    worst = 0.0
    for i, tr in enumerate(trace):
        col = i + 1
        if col < P:
            assert tr["next_ids"].view(B, K).cpu().tolist() == [[int(ids[b, col])] * K for b in range(B)]
            continue
        S, tok, par, info = hf_step(tr["logits"].cpu().view(B, K, V), S, col, P, cap, lp, es, EOS)
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
        if live.any():
            worst = max(worst, float((dev["run_scores"][live] - S["run_scores"][live]).abs().max()))
        assert int(tr["state"][3]) == int(bool(info["closed"].all()) or (i > 0 and int(trace[i - 1]["state"][3]))), (what, col)
        S["run_scores"], S["fin_scores"] = dev["run_scores"].clone(), dev["fin_scores"].clone()
    assert int(trace[-1]["state"][3]) == 1 and S["fin_flags"][:, 0].all(), what
    want = S["fin_seq"][:, 0, :P + int(S["fin_len"][:, 0].max())]
    assert torch.equal(out, want), what
    parity_log(f"beam replay {what}: {len(trace)} steps, max|running score - replay| {worst:.3e}, output {tuple(out.shape)}")
    return out


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("K,lp,es", SETTINGS)
def test_generate_beams_replays_through_transformers_helpers(dtype, K, lp, es):
    _, ours = _model(dtype, 2)
    pix = _pix(8, 64).to(DEV)
    out = _replay(ours, pix, K, lp, es, what=f"{dtype} K={K} lp={lp} es={es}")
    eager = ours.generate(pix, torch.tensor([PROMPT] * 8), max_new_tokens=12, num_beams=K, length_penalty=lp, early_stopping=es,
                          graph=False).cpu()
    assert torch.equal(out, eager), "graph replay must be bit-identical to graph=False"
    polled = ours.generate(pix, torch.tensor([PROMPT] * 8), max_new_tokens=12, num_beams=K, length_penalty=lp, early_stopping=es).cpu()
    assert torch.equal(out, polled), "steps run after the done word must not change the result"


# ---- 5. against transformers, fp16 -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [2, 3])
@pytest.mark.parametrize("K,lp,es", SETTINGS[:3])
def test_generate_beams_matches_transformers_fp16(seed, K, lp, es):
    """at most 1 of 8 rows may differ from the float32 oracle (a near-tie moved by fp16 logits); the search itself is checked by the
    replay, which runs here again for this very case"""
    ref, ours = _model("fp16", seed)
    pix = _pix(8, 64)
    prompt = torch.tensor([PROMPT] * 8)
    with torch.no_grad():
        want = ref.generate(pixel_values=pix, input_ids=prompt.clone(), max_new_tokens=12, num_beams=K, length_penalty=lp, early_stopping=es)
        greedy = ref.generate(pixel_values=pix, input_ids=prompt.clone(), max_new_tokens=12)
    n = min(want.shape[1], greedy.shape[1])
    assert want.shape != greedy.shape or (want[:, :n] != greedy[:, :n]).any(), "the oracle's beam output must differ from its greedy output"
    got = _replay(ours, pix.to(DEV), K, lp, es, what=f"fp16 seed={seed} K={K} lp={lp} es={es}")
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = (got != want).any(1).nonzero().flatten().tolist()
    for r in bad:
        c = int((got[r] != want[r]).nonzero()[0])
        parity_log(f"beam generate fp16 seed={seed} K={K} lp={lp} es={es}: row {r} first differs at generated step {c - (len(PROMPT) - 1)}")
    parity_log(f"beam generate fp16 seed={seed} K={K} lp={lp} es={es}: {len(bad)} of 8 rows differ from transformers")
    assert len(bad) <= 1, bad


# ---- 6. / 7. ---------------------------------------------------------------------------------------------------------------------

def test_beam_batch_independence():
    _, ours = _model("fp16", 2)
    pix = _pix(4, 64).to(DEV)
    prompt = torch.tensor([PROMPT] * 4)
    full = ours.generate(pix, prompt.clone(), max_new_tokens=10, num_beams=3).cpu()
    for i in range(4):
        one = ours.generate(pix[i:i + 1], prompt[i:i + 1].clone(), max_new_tokens=10, num_beams=3).cpu()[0]
        assert torch.equal(full[i, :one.numel()], one), i
        assert (full[i, one.numel():] == FILL).all(), i


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_greedy_is_untouched_by_a_beam_call(dtype):
    _, ours = _model(dtype, 2)
    pix = _pix(6, 64).to(DEV)
    prompt = torch.tensor([PROMPT] * 6)
    first = ours.generate(pix, prompt.clone(), max_new_tokens=12, num_beams=1).cpu()
    beams = ours.generate(pix, prompt.clone(), max_new_tokens=12, num_beams=3).cpu()
    again = ours.generate(pix, prompt.clone(), max_new_tokens=12).cpu()
    assert torch.equal(first, again)
    assert beams.shape[0] == 6 and (beams[:, :4] == first[:, :4]).all()
