"""GPU checks of the BLIP captioner (blip.BlipCaptioner) and its decode kernels (csrc/decode.hip) against float64 / the float32
transformers model.  Every measured deviation goes through conftest.parity_log."""
import pytest
import torch

transformers = pytest.importorskip("transformers")
from transformers import BlipForConditionalGeneration  # noqa: E402

from conftest import parity_log  # noqa: E402
from multimodal_propaganda_meme_classification_amd import BlipCaptioner, ops  # noqa: E402
from test_blip_caption import large_config, tiny_config  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
T16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
EOS, PAD = 102, 0


def _randomize(model, std, seed, eos_boost=0.0):
    """all weights N(0, std), LayerNorm weights 1 + N(0, 0.1): captions that depend on the image (the default initialisation of
    the vision tower, 1e-10, gives every image the same caption); eos_boost raises eos' bias so that some rows finish early"""
    g = torch.Generator().manual_seed(seed)
    sd = model.state_dict()
    with torch.no_grad():
        for k, v in sd.items():
            if v.dtype.is_floating_point:
                ln = k.endswith("weight") and any(s in k for s in ("LayerNorm", "layer_norm", "layernorm"))
                v.copy_((1 + 0.1 * torch.randn(v.shape, generator=g)) if ln else std * torch.randn(v.shape, generator=g))
        for k in ("text_decoder.cls.predictions.bias", "text_decoder.cls.predictions.decoder.bias"):
            sd[k][EOS] += eos_boost
    model.load_state_dict(sd)
    return model.eval()


def _pair(cfg, dtype="fp16", std=0.1, seed=1, eos_boost=1.0):
    ref = _randomize(BlipForConditionalGeneration(cfg), std, seed, eos_boost)
    ours = BlipCaptioner.from_config(cfg, compute_dtype=dtype, device=DEV)
    ours.load_state_dict(ref.state_dict(), strict=True)
    return ref, ours


def _pix(B, S, seed=3):
    return torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(seed))


# ---- mh_attn_decode ----------------------------------------------------------------------------------------------------------

def _attn64(q, k, v, T):
    """float64 reference: q [B, H, 64], k / v [B, T, H, 64]"""
    s = torch.einsum("bhd,bthd->bht", q.double(), k[:, :T].double()) / 8.0
    return torch.einsum("bht,bthd->bhd", torch.softmax(s, -1), v[:, :T].double())


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("BH", [(1, 2), (32, 12)])
def test_attn_decode_cross_against_float64(dtype, BH):
    B, H = BH
    D = H * 64
    worst = 0.0
    for T in (1, 2, 63, 64, 65, 127, 128, 129, 132, 577, 600):
        g = torch.Generator().manual_seed(T)
        q = torch.randn(B, D, generator=g).to(T16[dtype]).to(DEV)
        kv = (2 * torch.randn(B, T, 2 * D, generator=g)).to(T16[dtype]).to(DEV)      # [b][j][k | v]
        out = torch.full((B, D), float("nan"), dtype=T16[dtype], device=DEV)
        kf = kv.view(-1)
        ns = ops.decode_splits(B, H, T)
        ops.attn_decode(q, kf, kf[D:], out, B, H, T, D, T * 2 * D, 2 * D, D)
        ref = _attn64(q.cpu().view(B, H, 64), kv.cpu()[:, :, :D].view(B, T, H, 64), kv.cpu()[:, :, D:].view(B, T, H, 64), T)
        err = float((out.cpu().double().view(B, H, 64) - ref).abs().max())
        worst = max(worst, err)
        parity_log(f"attn_decode cross {dtype} B={B} H={H} T={T} nsplit={ns}: max|err|={err:.3e}")
        assert err <= (4e-3 if dtype == "fp16" else 3e-2) * max(1.0, float(ref.abs().max())), (T, err)
    if B * H < 256:
        assert ops.decode_splits(B, H, 600) > 1           # the split path ran


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("BH", [(1, 12), (64, 12)])
def test_attn_decode_self_cache_write_and_float64(dtype, BH):
    B, H = BH
    D, cap = H * 64, 140
    for t in (0, 1, 63, 64, 127, 128, 131, 139):
        g = torch.Generator().manual_seed(1000 + t)
        cache = torch.randn(B, cap, 2 * D, generator=g).to(T16[dtype]).to(DEV)
        before = cache.clone()
        qkv = torch.randn(B, 3 * D, generator=g).to(T16[dtype]).to(DEV)
        out = torch.empty((B, D), dtype=T16[dtype], device=DEV)
        tdev = torch.tensor([t], dtype=torch.int32, device=DEV)
        cf, qf = cache.view(-1), qkv.view(-1)
        ops.attn_decode(qkv, cf, cf[D:], out, B, H, cap, 3 * D, cap * 2 * D, 2 * D, D, t_dev=tdev, kv_new=qf[D:], ld_new=3 * D)
        c = cache.cpu()
        assert torch.equal(c[:, t], qkv.cpu()[:, D:]), "slot t must hold this step's k | v exactly"
        mask = torch.ones(cap, dtype=torch.bool)
        mask[t] = False
        assert torch.equal(c[:, mask], before.cpu()[:, mask]), "no other slot changes"
        ref = _attn64(qkv.cpu()[:, :D].view(B, H, 64), c[:, :, :D].view(B, cap, H, 64), c[:, :, D:].view(B, cap, H, 64), t + 1)
        err = float((out.cpu().double().view(B, H, 64) - ref).abs().max())
        parity_log(f"attn_decode self {dtype} B={B} H={H} t={t} nsplit={ops.decode_splits(B, H, cap)}: max|err|={err:.3e}")
        assert err <= (4e-3 if dtype == "fp16" else 3e-2) * max(1.0, float(ref.abs().max())), (t, err)
        out2 = torch.empty_like(out)
        ops.attn_decode(qkv, cf, cf[D:], out2, B, H, cap, 3 * D, cap * 2 * D, 2 * D, D, t_dev=tdev, kv_new=qf[D:], ld_new=3 * D)
        assert torch.equal(out, out2), "run to run bit-identical"


# ---- mh_greedy_step / mh_decode_embed ----------------------------------------------------------------------------------------

def test_greedy_step_ties_padding_eos_and_state():
    B, V, Vp, cap = 3, 300, 384, 6
    logits = torch.randn(B, Vp, generator=torch.Generator().manual_seed(0)).clamp(-3, 3)
    logits[0, 5] = logits[0, 17] = logits[0, 250] = 10.0        # a three-way tie: the lowest index wins
    logits[1, 40] = 9.0
    logits[1, V:] = 1e30                                         # padded columns never win
    logits[2, EOS] = 8.0
    logits = logits.to(DEV)
    out = torch.full((B, cap), PAD, dtype=torch.int64, device=DEV)
    out[:, 0] = 150
    nxt = torch.full((B,), 150, dtype=torch.int64, device=DEV)
    fin = torch.zeros(B, dtype=torch.int32, device=DEV)
    st = torch.zeros(4, dtype=torch.int32, device=DEV)
    ops.greedy_step(logits, V, out, nxt, fin, st, 1, EOS, PAD)
    assert out[:, 1].tolist() == [5, 40, EOS] and nxt.tolist() == [5, 40, EOS]
    assert fin.tolist() == [0, 0, 1] and st.tolist() == [1, 0, 1, 0]
    logits[0, EOS] = logits[1, EOS] = 20.0                      # rows 0 and 1 emit eos now; row 2 is finished: pad
    ops.greedy_step(logits, V, out, nxt, fin, st, 1, EOS, PAD)
    assert out[:, 2].tolist() == [EOS, EOS, PAD] and fin.tolist() == [1, 1, 1]
    assert st.tolist() == [2, 0, 3, 3]                           # all finished: output length 3
    ops.greedy_step(logits, V, out, nxt, fin, st, 1, EOS, PAD)
    assert out[:, 3].tolist() == [PAD] * 3 and st.tolist() == [3, 0, 3, 3]
    # inside the prompt: the next prompt token is copied, nothing finishes
    out2 = torch.tensor([[150, 7, 8, PAD, PAD]] * B, dtype=torch.int64, device=DEV)
    fin.zero_(), st.zero_()
    ops.greedy_step(logits, V, out2, nxt, fin, st, 3, EOS, PAD)
    assert out2[:, 1].tolist() == [7] * 3 and nxt.tolist() == [7] * 3 and fin.tolist() == [0] * 3 and st.tolist() == [1, 0, 0, 0]


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_decode_embed_against_float64(dtype):
    B, V, P, D = 5, 300, 64, 768
    g = torch.Generator().manual_seed(7)
    word, pos = torch.randn(V, D, generator=g), torch.randn(P, D, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    ids = torch.tensor([0, 5, 299, 102, 5], dtype=torch.int64)
    for t in (0, 5, 63):
        y = torch.empty(B, D, dtype=T16[dtype], device=DEV)
        ops.decode_embed(ids.to(DEV), torch.tensor([t], dtype=torch.int32, device=DEV), word.to(DEV), pos.to(DEV), gamma.to(DEV),
                         beta.to(DEV), 1e-12, y)
        ref = torch.nn.functional.layer_norm((word[ids] + pos[t]).double(), (D,), gamma.double(), beta.double(), 1e-12)
        err = float((y.cpu().double() - ref).abs().max())
        parity_log(f"decode_embed {dtype} t={t}: max|err|={err:.3e}")
        assert err <= (4e-3 if dtype == "fp16" else 3e-2) * float(ref.abs().max())


# ---- the model ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [64, 384])
def test_vision_tower_against_blip_vision_model(S):
    ref, ours = _pair(tiny_config(image_size=S))
    pix = _pix(2, S)
    with torch.no_grad():
        want = ref.vision_model(pixel_values=pix)[0]
    got = ours.vision_forward(pix.to(DEV)).float().cpu().view(want.shape)
    err = float((got - want).abs().max())
    rel = err / float(want.std())
    parity_log(f"blip vision tower fp16 {S}px ({want.shape[1]} tokens): max|err|={err:.3e} err/std={rel:.3e}")
    assert want.shape[1] == (S // 16) ** 2 + 1 and rel < 3e-2


def _oracle_logits(ref, pix, ids):
    with torch.no_grad():
        img = ref.vision_model(pixel_values=pix)[0]
        return ref.text_decoder(input_ids=ids, encoder_hidden_states=img).logits


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_decoder_teacher_forced_logits(dtype):
    ref, ours = _pair(tiny_config(), dtype)
    pix = _pix(3, 64)
    ids = torch.randint(0, 200, (3, 10), generator=torch.Generator().manual_seed(5))
    ids[:, 0] = 150
    want = _oracle_logits(ref, pix, ids)
    got = ours.teacher_forced_logits(pix.to(DEV), ids).cpu()
    err = float((got - want).abs().max())
    rel = err / float(want.std())
    parity_log(f"blip decoder teacher-forced logits {dtype}: max|err|={err:.3e} err/std={rel:.3e}")
    assert got.shape == want.shape and rel < (3e-2 if dtype == "fp16" else 1e-1)
    assert torch.equal(got, ours.teacher_forced_logits(pix.to(DEV), ids, graph=True).cpu()), "graph replay = eager, bitwise"


def _check_tokens(ref, ours, pix, prompt, got, want, what):
    """token-for-token equality; a mismatch is tolerated only where the oracle's top-2 logit margin at the first differing step is
    below the measured logits error"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if torch.equal(got, want):
        return
    bad = (got != want).any(1).nonzero().flatten().tolist()
    tf_ids = want[:, :-1].clone()
    lw = _oracle_logits(ref, pix, tf_ids)
    lg = ours.teacher_forced_logits(pix.to(DEV), tf_ids).cpu()
    err = float((lg - lw).abs().max())
    for r in bad:
        c = int((got[r] != want[r]).nonzero()[0])
        top2 = lw[r, c - 1].topk(2).values
        margin = float(top2[0] - top2[1])
        parity_log(f"{what}: row {r} differs at column {c}: oracle margin {margin:.3e} vs logits error {err:.3e}")
        assert margin < err, (what, r, c, margin, err)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_greedy_generate_matches_transformers(dtype):
    ref, ours = _pair(tiny_config(), dtype)
    pix = _pix(6, 64)
    prompt = torch.tensor([[101, 7, 8, 9, 102]] * 6)
    with torch.no_grad():
        want = ref.generate(pixel_values=pix, input_ids=prompt.clone(), max_new_tokens=12)
    assert len({tuple(r.tolist()) for r in want}) > 1, "the oracle's captions must depend on the image"
    eos_cols = [(r == EOS).nonzero().flatten().tolist() for r in want]
    assert any(c for c in eos_cols) and not all(c for c in eos_cols), "some rows end on eos before others"
    got = ours.generate(pix.to(DEV), prompt.clone(), max_new_tokens=12).cpu()
    parity_log(f"blip greedy generate {dtype}: {int((got != want).any(1).sum()) if got.shape == want.shape else 'shape'} of 6 rows differ")
    _check_tokens(ref, ours, pix, prompt, got, want, f"generate {dtype}")
    eager = ours.generate(pix.to(DEV), prompt.clone(), max_new_tokens=12, graph=False).cpu()
    assert torch.equal(got, eager), "graph replay must be bit-identical to graph=False"
    # all rows finish early: the output stops at the step where the last row emitted eos
    ref2, ours2 = _pair(tiny_config(), dtype, eos_boost=3.0)
    with torch.no_grad():
        want2 = ref2.generate(pixel_values=pix, input_ids=prompt.clone(), max_new_tokens=12)
    got2 = ours2.generate(pix.to(DEV), prompt.clone(), max_new_tokens=12, poll_every=3).cpu()
    assert want2.shape[1] < 4 + 12
    _check_tokens(ref2, ours2, pix, prompt, got2, want2, f"generate early-eos {dtype}")


def test_batch_independence():
    _, ours = _pair(tiny_config())
    pix = _pix(4, 64).to(DEV)
    prompt = torch.tensor([[101, 7, 8, 9, 102]] * 4)
    full = ours.generate(pix, prompt.clone(), max_new_tokens=10).cpu()
    for i in range(4):
        one = ours.generate(pix[i:i + 1], prompt[i:i + 1].clone(), max_new_tokens=10).cpu()[0]
        assert torch.equal(full[i, :one.numel()], one), i
        assert (full[i, one.numel():] == PAD).all(), i


def test_blip_large_dimensions_teacher_forced():
    cfg = large_config()
    torch.manual_seed(0)
    with torch.device(DEV):
        ref = BlipForConditionalGeneration(cfg)
    _randomize(ref, 0.02, 11)
    ours = BlipCaptioner.from_config(cfg, device=DEV)
    ours.load_state_dict(ref.state_dict(), strict=True)
    pix = _pix(4, 384).to(DEV)
    ids = torch.randint(0, 30524, (4, 6), generator=torch.Generator().manual_seed(2)).to(DEV)
    ids[:, 0] = 30522
    want = _oracle_logits(ref, pix, ids).float()
    got = ours.teacher_forced_logits(pix, ids)
    err = float((got - want).abs().max())
    rel = err / float(want.std())
    parity_log(f"blip-large dims teacher-forced logits fp16 (24-layer ViT-L/16 @ 384, 12-layer decoder): max|err|={err:.3e} err/std={rel:.3e}")
    assert rel < 5e-2


# ---- history independence of the decode state -----------------------------------------------------------------------------------
# BlipCaptioner keeps one decode state per (B, cap, K): the self-attention cache (zeroed only at allocation), the cross k / v, the
# beam ancestry table, and a captured step keyed by (P, num_beams, length_penalty, early_stopping).  A call's result is a function of
# the weights and its own arguments, never of the call before it.

def _gen_len(row, P):
    """generated tokens of one returned row up to and including the first eos (the whole tail when there is none)"""
    hit = (row[P:] == EOS).nonzero().flatten()
    return int(hit[0]) + 1 if hit.numel() else row.numel() - P


def _short_and_long(cfg, sd, dtype, pix, prompt, kw_x, kw_y):
    """two images whose captions under kw_x are the shortest and two whose captions under kw_y are the longest of the sixteen, found
    with a captioner of their own; the generated lengths (x, y) come back for the record"""
    scout = BlipCaptioner.from_config(cfg, compute_dtype=dtype, device=DEV)
    scout.load_state_dict(sd, strict=True)
    P = prompt.shape[1] - 1
    def lengths(kw):        # eight images a call
        return torch.tensor([_gen_len(r, P) for i in range(0, pix.shape[0], 8)
                             for r in scout.generate(pix[i:i + 8].to(DEV), prompt[i:i + 8].clone(), max_new_tokens=12, **kw).cpu()])

    lx, ly = lengths(kw_x), lengths(kw_y)
    parity_log(f"blip history scout {dtype}: generated lengths under X's arguments {lx.tolist()}, under Y's {ly.tolist()}")
    ix, iy = lx.argsort(stable=True)[:2], ly.argsort(stable=True)[-2:]
    return ix, iy, lx[ix].tolist(), ly[iy].tolist()


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("case", ["greedy-after-greedy", "beams-after-beams-other-length-penalty", "greedy-after-beams"])
def test_generate_does_not_depend_on_the_call_before(dtype, case):
    """generate(Y) then generate(X) on one captioner equals a fresh captioner's generate(X) token for token, and
    teacher_forced_logits after them equals a fresh captioner's bit for bit.  Y has X's batch size and cap (and, in the first two
    cases, its beam count: the same decode state) and runs LONGER than X -- asserted from the returned lengths -- so the cache and
    the sequences hold Y's tokens beyond where X stops.  Beams after beams with another length_penalty re-captures the step."""
    kw_x, kw_y = {"greedy-after-greedy": ({}, {}),
                  "beams-after-beams-other-length-penalty": (dict(num_beams=3, length_penalty=1.0), dict(num_beams=3, length_penalty=2.0)),
                  "greedy-after-beams": ({}, dict(num_beams=3))}[case]
    cfg = tiny_config()
    ref = _randomize(BlipForConditionalGeneration(cfg), 0.1, 1, 1.0)
    sd = ref.state_dict()

    def captioner():
        c = BlipCaptioner.from_config(cfg, compute_dtype=dtype, device=DEV)
        c.load_state_dict(sd, strict=True)
        return c

    pix = _pix(16, 64, seed=21)
    prompt = torch.tensor([[101, 7, 8, 9, 102]] * 16)
    ix, iy, len_x, len_y = _short_and_long(cfg, sd, dtype, pix, prompt, kw_x, kw_y)
    parity_log(f"blip history {case} {dtype}: generated lengths X {len_x} (images {ix.tolist()}), Y {len_y} (images {iy.tolist()})")
    px, py, p2 = pix[ix].to(DEV), pix[iy].to(DEV), prompt[:2]
    used, fresh, fresh_tf = captioner(), captioner(), captioner()
    got_y = used.generate(py, p2.clone(), max_new_tokens=12, **kw_y).cpu()
    got_x = used.generate(px, p2.clone(), max_new_tokens=12, **kw_x).cpu()
    want_x = fresh.generate(px, p2.clone(), max_new_tokens=12, **kw_x).cpu()
    assert got_y.shape[1] > got_x.shape[1], ("Y has to run longer than X", got_y.shape, got_x.shape)
    assert got_x.shape == want_x.shape and torch.equal(got_x, want_x), (case, got_x.tolist(), want_x.tolist())
    if not kw_x and not kw_y:
        assert len(used._states) == 1 and next(iter(used._states))[:2] == (2, 4 + 12), "X and Y share one decode state"
    # teacher forcing over cap - 1 tokens: the greedy state of (B, cap) again
    ids = torch.randint(0, 200, (2, 4 + 12 - 1), generator=torch.Generator().manual_seed(6))
    ids[:, 0] = 150
    tf_used, tf_fresh = used.teacher_forced_logits(px, ids), fresh_tf.teacher_forced_logits(px, ids)
    assert tf_used.shape == tf_fresh.shape and torch.equal(tf_used.view(torch.int32), tf_fresh.view(torch.int32))
    assert bool(torch.isfinite(tf_fresh).all())
