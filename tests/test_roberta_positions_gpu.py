"""RoBERTa-family text towers on the device (TextConfig.position_scheme = "roberta"; include/memehip.h: mh_position_ids_from_input_ids,
mh_bert_embed_fwd_pos, mh_embed_pos_bwd).

  1. position ids / inverse map      exact against an integer restatement in torch, on both sides of the 64-lane trip
  2. forward with position ids       float64 with the bars of test_layer_paths_gpu.py::test_bert_embed_forward; without pad tokens
                                       bit-identical to mh_bert_embed_fwd on the table shifted by pad_id + 1 rows
  3. position / token-type backward  bit-identical to mh_bert_embed_bwd where both sum the same rows; float64 (_check_sum) with
                                       gradient-carrying pad tokens; every row written; reproducible
  4. golden (transformers RobertaModel, tests/golden/roberta_tiny.npz): position ids exact, pre / y within the _check16 bars,
                                       table gradients within the _check_sum bar + the rounding of d_pre to 16 bits
  5. tower                           the roberta-scheme model == its absolute-scheme twin (table shifted) bit for bit: logits,
                                       pooled features, every gradient -- the twin is what the existing goldens pin to BertModel
  6. captured step                   GraphedStep replayed on batches with different pad patterns == the eager step, bit for bit
  7. checkpoint and Kevin's model    a RobertaModel state dict loads strictly; KevinMultimodalClassifier with a roberta caption tower
"""
import os

import numpy as np
import pytest
import torch

from conftest import parity_log
from test_layer_paths_gpu import (DTYPES, F16, F32, F64, I32, I64, SENT32, TOL_SUM, _check16, _check_sum, _cpu, _dev, _eps,
                                  _ln_params, _ln_stats, _name, _r16, _rand, _rng, _same_bits, _sent16)

pytestmark = pytest.mark.gpu

KINDS = ("none", "right", "left", "interior", "all")


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.set_num_threads(16)
    import multimodal_propaganda_meme_classification_amd as m
    from multimodal_propaganda_meme_classification_amd import ops as _ops
    m.ops = _ops
    return m


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "roberta_tiny.npz"))


def _row(kind, S, V, pad, g):
    """One row of ids in [0, V) without `pad`, then padded as `kind` says."""
    ids = torch.randint(0, V - 1, (S,), generator=g)
    ids = ids + (ids >= pad).long()
    n = int(torch.randint(1, S + 1, (1,), generator=g)) if S > 1 else 1
    if kind == "right":
        ids[n:] = pad
    elif kind == "left":
        ids[:S - n] = pad
    elif kind == "interior":
        ids[torch.rand(S, generator=g) < 0.3] = pad
        if S > 2:
            ids[S // 2] = pad
    elif kind == "all":
        ids[:] = pad
    return ids


def _ids(kinds, S, V, pad, g):
    return torch.stack([_row(k, S, V, pad, g) for k in kinds])


def _positions(ids, pad, P):
    """The rule in torch integers: (pos_ids [B,S], pos_inv [B,P]); an id past the table is clamped and left out of pos_inv."""
    live = ids != pad
    pos = torch.where(live, pad + live.long().cumsum(1), torch.full_like(ids, pad))
    inv = torch.full((ids.shape[0], P), -1, dtype=I64)
    b, s = torch.nonzero(live & (pos < P), as_tuple=True)
    inv[b, pos[b, s]] = s
    return pos.clamp(max=P - 1).to(I32), inv.to(I32)


# ---- 1. position ids and inverse map ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("B", [1, 3, 17])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 130])
def test_position_ids_and_inverse_map(pkg, S, B, pad):
    g = torch.Generator().manual_seed(1000 * S + 10 * B + pad)
    P = S + pad + 2                       # one row more than the longest sequence reads
    for rot in range(1 if B >= len(KINDS) else len(KINDS)):         # small batches: every kind of row in turn
        ids = _ids([KINDS[(b + rot) % len(KINDS)] for b in range(B)], S, 300, pad, g)
        want_pos, want_inv = _positions(ids, pad, P)
        for kind in ("bf16", "fp16"):     # the kernel is untyped; both libraries export it
            pos_ids = torch.full((B, S), -77, dtype=I32, device="cuda")
            pos_inv = torch.randint(-5, 1000, (B, P), dtype=I32, device="cuda")          # garbage: every entry must be written
            got = pkg.ops.position_ids_from_input_ids(ids.cuda(), pad, P, pos_ids=pos_ids, pos_inv=pos_inv, kind=kind)
            torch.cuda.synchronize()
            assert got[0] is pos_ids and got[1] is pos_inv
            assert torch.equal(pos_ids.cpu(), want_pos), (kind, rot)
            assert torch.equal(pos_inv.cpu(), want_inv), (kind, rot)
            assert bool((pos_inv[:, :pad + 1] == -1).all())


def test_position_ids_stay_inside_a_short_table(pkg):
    """Unreachable from the model (config.check_sequence_length); the kernel still clamps instead of leaving the table."""
    g = torch.Generator().manual_seed(5)
    S, pad, P = 70, 1, 40
    ids = _ids(["none", "right", "left", "interior", "none"], S, 300, pad, g)
    want_pos, want_inv = _positions(ids, pad, P)
    assert int(want_pos.max()) == P - 1 and int((want_pos == P - 1).sum()) > 40
    guard = torch.full((ids.shape[0] + 1, P), 12345, dtype=I32, device="cuda")
    pos_ids, pos_inv = pkg.ops.position_ids_from_input_ids(ids.cuda(), pad, P, pos_inv=guard[:-1])
    torch.cuda.synchronize()
    assert torch.equal(pos_ids.cpu(), want_pos) and torch.equal(pos_inv.cpu(), want_inv)
    assert bool((guard[-1] == 12345).all())


# ---- 2. forward -------------------------------------------------------------------------------------------------------------------

def _fwd_buffers(T, D, T16):
    return (_sent16((T, D), T16), _sent16((T, D), T16), torch.full((T,), SENT32, dtype=F32, device="cuda"),
            torch.full((T,), SENT32, dtype=F32, device="cuda"))


@DTYPES
@pytest.mark.parametrize("has_type", [True, False], ids=["type0", "notype"])
@pytest.mark.parametrize("D", [128, 768])
def test_embed_forward_with_position_ids(pkg, D, has_type, T16):
    B, S, V, pad, eps = 5, 40, 300, 1, 1e-5
    g = torch.Generator().manual_seed(D + S + int(has_type))
    P = S + pad + 1 + 3
    ids = _ids(["none", "right", "left", "interior", "right"], S, V, pad, g)
    word = (0.05 * _rand((V, D), g)).to(F32)
    pos = (0.02 * _rand((P, D), g)).to(F32)
    type0 = (0.02 * _rand((D,), g)).to(F32) if has_type else None
    gamma, beta = _ln_params(D, g)
    dev = lambda t: None if t is None else t.to(F32).cuda()
    T = B * S
    pos_ids, _ = pkg.ops.position_ids_from_input_ids(ids.cuda(), pad, P)
    pre, y, mean, rstd = _fwd_buffers(T, D, T16)
    pkg.ops.bert_embed_fwd_pos(ids.cuda(), pos_ids, dev(word), dev(pos), dev(type0), dev(gamma), dev(beta), eps, pre, y, mean, rstd)
    torch.cuda.synchronize()
    want_pos, _ = _positions(ids, pad, P)
    assert torch.equal(pos_ids.cpu(), want_pos)
    w64 = word.to(F64)[ids.flatten()]
    p64 = pos.to(F64)[want_pos.flatten().long()]
    v = w64 + p64
    terms = w64.abs() + p64.abs()
    if type0 is not None:
        v = v + type0.to(F64)
        terms = terms + type0.to(F64).abs()
    tag = f"embed_pos D{D} type0={int(has_type)} {_name(T16)}"
    errs = {"pre": _check16(f"{tag} pre", pre, v, T16, TOL_SUM * terms)}
    mu, rs = _ln_stats(v, eps)
    m_k, r_k = _cpu(mean), _cpu(rstd)
    errs["mean"] = _check_sum(f"{tag} mean", mean, mu, v.abs().mean(1))
    rel = float(((r_k - rs).abs() / rs).max())
    assert rel <= _eps(T16) / 2, f"{tag} rstd: relative error {rel:.3g} > EPS/2"
    d = v - m_k[:, None]
    yv = d * r_k[:, None] * gamma + beta
    yterms = (d.abs() + terms) * r_k[:, None] * gamma.abs() + beta.abs()
    errs["y"] = _check16(f"{tag} y", y, yv, T16, TOL_SUM * yterms)
    parity_log(f"[roberta {tag}] " + " ".join(f"{k} {x:.3e}" for k, x in errs.items()))

    # without pad tokens: the same bits as the absolute kernel on the table shifted by pad + 1 rows (dropout on, same site)
    ids2 = _ids(["none"] * B, S, V, pad, g).cuda()
    drop = (_rng(11, 4), 0.1, 3)
    pos_ids2, _ = pkg.ops.position_ids_from_input_ids(ids2, pad, P)
    a, b = _fwd_buffers(T, D, T16), _fwd_buffers(T, D, T16)
    pkg.ops.bert_embed_fwd_pos(ids2, pos_ids2, dev(word), dev(pos), dev(type0), dev(gamma), dev(beta), eps, *a, drop=drop)
    pkg.ops.bert_embed_fwd(ids2, dev(word), dev(pos)[pad + 1:].contiguous(), dev(type0), dev(gamma), dev(beta), eps, *b, drop=drop)
    torch.cuda.synchronize()
    for name, x, z in zip(("pre", "y", "mean", "rstd"), a, b):
        assert _same_bits(x, z), f"{tag}: {name} differs from mh_bert_embed_fwd on the shifted table"


# ---- 3. backward ------------------------------------------------------------------------------------------------------------------

BWD = {"B19_S24_D136": (19, 24, 136), "B3_S70_D768": (3, 70, 768)}       # (B, S, D): more samples than one 16-sample trip / S > 64


def _pos_bwd(pkg, d16, pos_inv, P, D, S, scale, fill=float("nan"), with_type=True):
    dpos = torch.full((P, D), fill, dtype=F32, device="cuda")
    dtype0 = torch.full((D,), fill, dtype=F32, device="cuda") if with_type else None
    scratch = torch.full((S, D), fill, dtype=F32, device="cuda") if with_type else None
    pkg.ops.embed_pos_bwd(d16, pos_inv, dpos, dtype0, scratch, scale=scale)
    torch.cuda.synchronize()
    return dpos, dtype0


@DTYPES
@pytest.mark.parametrize("size", list(BWD))
def test_position_backward_equals_the_absolute_kernel(pkg, size, T16):
    """No pad, and right pad with a zero gradient on the pad rows: both kernels sum the same rows, in the same order."""
    B, S, D = BWD[size]
    V, pad, scale = 97, 1, 0.37
    P = S + pad + 1 + 2
    g = torch.Generator().manual_seed(B + D)
    for kinds in (["none"] * B, ["right" if b % 3 else "none" for b in range(B)]):
        ids = _ids(kinds, S, V, pad, g)
        d = _r16(_rand((B, S, D), g, 4.0), T16)
        d[ids == pad] = 0.0
        d16 = _dev(d.view(B * S, D), T16)
        _, pos_inv = pkg.ops.position_ids_from_input_ids(ids.cuda(), pad, P)
        dpos, dtype0 = _pos_bwd(pkg, d16, pos_inv, P, D, S, scale)
        dword = torch.zeros((V, D), dtype=F32, device="cuda")
        ref_pos = torch.full((S, D), SENT32, dtype=F32, device="cuda")
        ref_type = torch.full((D,), SENT32, dtype=F32, device="cuda")
        pkg.ops.bert_embed_bwd(ids.cuda(), d16, dword, ref_pos, ref_type, pad, scale=scale)
        torch.cuda.synchronize()
        assert _same_bits(dpos[pad + 1:pad + 1 + S], ref_pos), f"{size} {kinds[1]}: dpos differs from mh_bert_embed_bwd"
        assert _same_bits(dtype0, ref_type), f"{size} {kinds[1]}: dtype0 differs from mh_bert_embed_bwd"
        assert bool((dpos[:pad + 1] == 0).all()) and bool((dpos[pad + 1 + S:] == 0).all())
        # without dtype0 the position rows are the same
        dpos2, _ = _pos_bwd(pkg, d16, pos_inv, P, D, S, scale, with_type=False)
        assert _same_bits(dpos2, dpos)


@DTYPES
@pytest.mark.parametrize("size", list(BWD))
def test_position_backward_with_gradient_on_pad_tokens(pkg, size, T16):
    B, S, D = BWD[size]
    pad, scale = 1, 0.37
    P = S + pad + 1 + 2
    g = torch.Generator().manual_seed(B + D + 1)
    ids = _ids([("interior", "left", "none", "right")[b % 4] for b in range(B)], S, 97, pad, g)
    d = _r16(_rand((B, S, D), g, 4.0), T16)             # non-zero everywhere, pad tokens included
    d16 = _dev(d.view(B * S, D), T16)
    pos, pos_inv = pkg.ops.position_ids_from_input_ids(ids.cuda(), pad, P)
    dpos, dtype0 = _pos_bwd(pkg, d16, pos_inv, P, D, S, scale)
    live = (ids != pad).flatten()
    rows = pos.cpu().flatten().long()[live]
    ref = torch.zeros((P, D), dtype=F64).index_add_(0, rows, d.view(-1, D)[live]) * scale
    terms = torch.zeros((P, D), dtype=F64).index_add_(0, rows, d.view(-1, D)[live].abs()) * scale
    tag = f"pos_bwd {size} {_name(T16)}"
    errs = {"dpos": _check_sum(f"{tag} dpos", dpos, ref, terms)}
    untouched = torch.ones(P, dtype=torch.bool)
    untouched[rows] = False
    assert untouched[:pad + 1].all() and int(untouched.sum()) >= pad + 2
    assert bool((dpos.cpu()[untouched] == 0).all()), "a row no token reads is not exactly zero (dpos was pre-filled with NaN)"
    assert int((~live).sum()) > B and float(d.view(-1, D)[~live].abs().min()) > 0        # the pad tokens did carry gradient
    # ... and all of it reaches the token-type row
    errs["dtype0"] = _check_sum(f"{tag} dtype0", dtype0, scale * d.sum((0, 1)), scale * d.abs().sum((0, 1)))
    again = _pos_bwd(pkg, d16, pos_inv, P, D, S, scale, fill=-3.0)
    assert _same_bits(again[0], dpos) and _same_bits(again[1], dtype0), "two calls give different bits"
    parity_log(f"[roberta {tag}] " + " ".join(f"{k} {x:.3e}" for k, x in errs.items()))


# ---- 4. golden ----------------------------------------------------------------------------------------------------------------------

def _golden_cfg(pkg, golden, **kw):
    """The fixture's RobertaConfig as a TextConfig."""
    V, D = golden["p:embeddings.word_embeddings.weight"].shape
    return pkg.TextConfig(vocab_size=V, hidden=D, layers=1, heads=2, intermediate=128, max_position=24, type_vocab=1, pad_token_id=1,
                          ln_eps=1e-5, position_scheme="roberta", **kw)


def _golden_sd(golden):
    return {k[2:]: torch.from_numpy(golden[k]) for k in golden.files if k.startswith("p:")}


@DTYPES
def test_golden_embeddings_and_table_gradients(pkg, golden, T16):
    ids = torch.from_numpy(golden["ids"])
    B, S = ids.shape
    pad, eps = 1, 1e-5
    sd = _golden_sd(golden)
    word, pos, type0 = (sd[f"embeddings.{n}.weight"] for n in ("word_embeddings", "position_embeddings", "token_type_embeddings"))
    gamma, beta = sd["embeddings.LayerNorm.weight"], sd["embeddings.LayerNorm.bias"]
    P, D = pos.shape
    pos_ids, pos_inv = pkg.ops.position_ids_from_input_ids(ids.cuda(), pad, P)
    assert torch.equal(pos_ids.cpu(), torch.from_numpy(golden["position_ids"]))
    pre, y, mean, rstd = _fwd_buffers(B * S, D, T16)
    pkg.ops.bert_embed_fwd_pos(ids.cuda(), pos_ids, word.cuda(), pos.cuda(), type0[0].contiguous().cuda(), gamma.cuda(), beta.cuda(), eps,
                               pre, y, mean, rstd)
    torch.cuda.synchronize()
    w64, p64, t64 = word.to(F64)[ids.flatten()], pos.to(F64)[pos_ids.cpu().flatten().long()], type0[0].to(F64)
    terms = w64.abs() + p64.abs() + t64.abs()
    v = torch.from_numpy(golden["pre"]).to(F64).view(B * S, D)
    tag = f"golden {_name(T16)}"
    errs = {"pre": _check16(f"{tag} pre", pre, v, T16, TOL_SUM * terms)}
    mu, rs = _ln_stats(v, eps)
    dd = v - mu[:, None]
    yterms = (dd.abs() + terms) * rs[:, None] * gamma.to(F64).abs() + beta.to(F64).abs()
    errs["y"] = _check16(f"{tag} y", y, torch.from_numpy(golden["emb_out"]).to(F64).view(B * S, D), T16, TOL_SUM * yterms)

    # table gradients from transformers' d_pre rounded to 16 bits.  fp16 carries gradients under a power-of-two stream scale (the
    # model's grad_stream_scale): the largest that keeps the fixture's values finite, so that rounding stays relative (eps/2).
    d = torch.from_numpy(golden["d_pre"]).to(F64)
    k = 2.0 ** int(np.floor(np.log2(30000.0 / float(d.abs().max())))) if T16 == F16 else 1.0
    d16 = (d * k).to(T16)
    assert bool(((d16.to(F64) / k - d).abs() <= _eps(T16) / 2 * d.abs()).all()), "the 16-bit rounding of d_pre is not relative"
    half = _eps(T16) / 2
    dpos = torch.full((P, D), float("nan"), dtype=F32, device="cuda")
    dtype0, scratch = torch.empty(D, dtype=F32, device="cuda"), torch.empty((S, D), dtype=F32, device="cuda")
    pkg.ops.embed_pos_bwd(d16.view(B * S, D).cuda(), pos_inv, dpos, dtype0, scratch, scale=1.0 / k)
    V = word.shape[0]
    dword, junk = torch.zeros((V, D), dtype=F32, device="cuda"), torch.empty((S, D), dtype=F32, device="cuda")
    pkg.ops.bert_embed_bwd(ids.cuda(), d16.view(B * S, D).cuda(), dword, junk, None, pad, scale=1.0 / k)
    torch.cuda.synchronize()
    flat, live = d.view(B * S, D).abs(), (ids != pad).flatten()
    rows = pos_ids.cpu().flatten().long()
    t_pos = torch.zeros((P, D), dtype=F64).index_add_(0, rows[live], flat[live])
    t_word = torch.zeros((V, D), dtype=F64).index_add_(0, ids.flatten()[live], flat[live])
    t_type = flat.sum(0)
    errs["g_pos"] = _check_sum(f"{tag} g_pos", dpos, torch.from_numpy(golden["g_pos"]).to(F64), t_pos, extra=half * t_pos)
    errs["g_type"] = _check_sum(f"{tag} g_type", dtype0, torch.from_numpy(golden["g_type"][0]).to(F64), t_type, extra=half * t_type)
    errs["g_word"] = _check_sum(f"{tag} g_word", dword, torch.from_numpy(golden["g_word"]).to(F64), t_word, extra=half * t_word)
    assert bool((dpos[pad] == 0).all()) and bool((dword[pad] == 0).all())
    parity_log(f"[roberta {tag}] " + " ".join(f"{k_} {x:.3e}" for k_, x in errs.items()))


# ---- 5. the tower against its absolute-scheme twin ---------------------------------------------------------------------------------------

def _tiny_text(pkg, scheme, max_position):
    return pkg.TextConfig(vocab_size=256, hidden=128, layers=1, heads=2, intermediate=128, max_position=max_position, type_vocab=1,
                          pad_token_id=1, ln_eps=1e-5, position_scheme=scheme)


def _tiny_model(pkg, scheme, max_position, dtype, pack=True, seed=7):
    cfg = pkg.ModelConfig(text=_tiny_text(pkg, scheme, max_position),
                          image=pkg.ImageConfig(image_size=32, patch=16, hidden=128, layers=1, heads=2, intermediate=128),
                          proj=128, num_classes=2, pool="cls", compute_dtype=dtype, pack_text=pack)
    return pkg.MultimodalClassifier.from_config(cfg, seed=seed)


POS = "bert.embeddings.position_embeddings.weight"


def _batch(B, S, kinds, seed, pad=1):
    g = torch.Generator().manual_seed(seed)
    ids = _ids(kinds, S, 256, pad, g)
    ids[:, 0] = 0                                   # <s>: the pooled token is never a pad
    image = torch.randn((B, 3, 32, 32), generator=g)
    labels = torch.randint(0, 2, (B,), generator=g)
    return ids, image, labels


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("pack", [True, False], ids=["packed", "dense"])
def test_tower_equals_its_absolute_twin(pkg, pack, dtype):
    B, S, pad = 3, 16, 1
    rob = _tiny_model(pkg, "roberta", 24, dtype, pack)
    twin = _tiny_model(pkg, "absolute", 16, dtype, pack)
    sd = {k: v.detach().clone() for k, v in rob.state_dict().items()}
    sd[POS] = sd[POS][pad + 1:pad + 1 + S].clone()
    twin.load_state_dict(sd)
    rob.cuda().train(), twin.cuda().train()
    ids, image, labels = _batch(B, S, ["right", "none", "right"], 11)
    mask = (ids != pad).long()
    assert 0 < int((mask == 0).sum()) and bool(mask[1].all())
    dev = [t.cuda() for t in (ids, image, mask, labels)]
    out = []
    for m in (rob, twin):
        with torch.no_grad():
            feats = m.encode(*dev[:3])[0].clone()
        loss, _, logits = m.forward_backward(*dev)
        torch.cuda.synchronize()
        out.append((feats, logits.clone(), loss.clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}))
    (f_r, l_r, loss_r, g_r), (f_t, l_t, loss_t, g_t) = out
    assert torch.equal(f_r, f_t), "pooled text features differ"
    assert torch.equal(l_r, l_t) and torch.equal(loss_r, loss_t), "logits / loss differ"
    assert bool(torch.isfinite(l_r).all()) and float(g_r[POS].abs().sum()) > 0
    assert sorted(g_r) == sorted(g_t)
    for n in g_r:
        if n == POS:
            assert torch.equal(g_r[n][pad + 1:pad + 1 + S], g_t[n]), "position-table gradient differs (row-shifted)"
            assert bool((g_r[n][:pad + 1] == 0).all()) and bool((g_r[n][pad + 1 + S:] == 0).all())
        else:
            assert torch.equal(g_r[n], g_t[n]), f"gradient of {n} differs"
    names = [c.name for c in rob._get_engine().plan(B, S).fwd.calls[:2]]
    assert names == ["mh_position_ids_from_input_ids", "mh_bert_embed_fwd_pos"], names
    assert twin._get_engine().plan(B, S).fwd.calls[0].name == "mh_bert_embed_fwd"


def test_sequence_too_long_for_the_table_raises_before_any_launch(pkg):
    m = _tiny_model(pkg, "roberta", 24, "bf16").cuda()
    ids, image, labels = _batch(2, 23, ["none", "right"], 3)           # 23 + 1 + 1 > 24
    with pytest.raises(ValueError, match="max_position 24"):
        m(ids.cuda(), image.cuda(), (ids != 1).long().cuda())


# ---- 6. captured step --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_graphed_step_replays_other_pad_patterns(pkg, dtype):
    """The position ids are computed inside the captured forward from the static ids buffer: one graph, any batch."""
    B, S, pad = 4, 16, 1
    m_graph, m_eager = _tiny_model(pkg, "roberta", 24, dtype), _tiny_model(pkg, "roberta", 24, dtype)
    m_graph.cuda().train(), m_eager.cuda().train()
    o_graph = pkg.Adam(m_graph.parameters(), lr=1e-3, model=m_graph)
    o_eager = pkg.Adam(m_eager.parameters(), lr=1e-3, model=m_eager)
    gs = pkg.GraphedStep(m_graph, o_graph, B, S, use_graph=True)
    scaler = gs.scaler
    if scaler is not None:                       # fp16: the eager model runs under the same dynamic loss scale
        scaler = pkg.GradScaler()
        scaler.attach_model(m_eager)
    try:
        seen = []
        for step, (kinds, full_mask) in enumerate(((["right", "none", "right", "right"], False),
                                                    (["interior", "left", "none", "interior"], True),
                                                    (["right", "right", "interior", "none"], False))):
            ids, image, labels = _batch(B, S, kinds, 40 + step)
            if full_mask:
                ids[1, 0] = pad                   # a left-padded row keeps its pad at the pooled position
            mask = torch.ones_like(ids) if full_mask else (ids != pad).long()
            mask[:, 0] = 1
            dev = [t.cuda() for t in (ids, image, mask, labels)]
            gs.load_batch(*dev)
            loss_g, _ = gs.step()
            loss_e, _, _ = m_eager.forward_backward(*dev)
            if scaler is not None:
                scaler.step(o_eager)
                scaler.update()
            else:
                o_eager.step()
            torch.cuda.synchronize()
            assert torch.equal(gs.plan.buf["t.pos_ids"].cpu(), _positions(ids, pad, 24)[0]), step
            assert float(loss_g) == float(loss_e) and np.isfinite(float(loss_g)), (step, float(loss_g), float(loss_e))
            assert torch.equal(m_graph.flat_params, m_eager.flat_params), f"parameters differ after step {step}"
            assert torch.equal(m_graph.flat_grads, m_eager.flat_grads), f"gradients differ after step {step}"
            seen.append(tuple(gs.plan.buf["t.pos_ids"].flatten().tolist()))
        assert len(set(seen)) == 3
        assert gs.use_graph and gs.graphs is not None and len(gs.graphs) == 1, "the step did not replay ONE hipGraph"
    finally:
        gs.close()


# ---- 7. checkpoint and Kevin's model ------------------------------------------------------------------------------------------------------

def test_roberta_state_dict_loads_strictly(pkg, golden):
    sd = _golden_sd(golden)
    ckpt = dict(sd)
    ckpt["embeddings.position_ids"] = torch.arange(24)[None]          # buffers older transformers versions persist
    ckpt["embeddings.token_type_ids"] = torch.zeros((1, 24), dtype=torch.long)
    enc = pkg.TextEncoder(_golden_cfg(pkg, golden), pool="cls", compute_dtype="bf16")
    res = enc.load_state_dict(ckpt, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    back = enc.state_dict()
    assert sorted(back) == sorted(sd)
    for k_, v in sd.items():
        assert torch.equal(back[k_].detach().cpu(), v), k_
    with pytest.raises(RuntimeError):
        enc.load_state_dict(dict(ckpt, **{"embeddings.unknown.weight": torch.zeros(1)}), strict=True)

    # recorded, not asserted: the whole encoder against transformers, next to the absolute twin on the rows both can state
    ids, mask = torch.from_numpy(golden["ids"]).cuda(), torch.from_numpy(golden["mask"]).cuda()
    want = torch.from_numpy(golden["last_hidden_state"])
    twin_sd = dict(sd)
    twin_sd["embeddings.position_embeddings.weight"] = sd["embeddings.position_embeddings.weight"][2:18].clone()
    for dtype in ("bf16", "fp16"):
        enc = pkg.TextEncoder(_golden_cfg(pkg, golden), compute_dtype=dtype)
        enc.load_state_dict(sd)
        twin = pkg.TextEncoder(pkg.TextConfig(vocab_size=256, hidden=128, layers=1, heads=2, intermediate=128, max_position=16,
                                              type_vocab=1, pad_token_id=1, ln_eps=1e-5), compute_dtype=dtype)
        twin.load_state_dict(twin_sd)
        with torch.no_grad():
            h = enc.cuda().eval().hidden_states(ids, mask).float().cpu()
            ht = twin.cuda().eval().hidden_states(ids, mask).float().cpu()
        assert bool(torch.isfinite(h).all())
        live = mask.cpu().bool()
        e_all = float((h - want)[live].abs().max())
        e_01 = float((h - want)[:2][live[:2]].abs().max())           # rows 0 / 1: no pad, right pad
        e_twin = float((ht - want)[:2][live[:2]].abs().max())
        parity_log(f"[roberta hidden_states {dtype}] max |hip - transformers| over attended positions: roberta scheme {e_all:.3e} "
                   f"(4 rows), {e_01:.3e} (rows without / with right padding); absolute twin on those two rows {e_twin:.3e}; "
                   f"max |last_hidden_state| {float(want.abs().max()):.3f}")


def test_kevin_model_with_a_roberta_caption_tower(pkg, golden):
    B, S = 4, 16
    tc = pkg.TextConfig(vocab_size=300, hidden=128, layers=1, heads=2, intermediate=128, max_position=32)
    ic = pkg.ImageConfig(image_size=32, patch=16, hidden=128, layers=1, heads=2, intermediate=128)
    model = pkg.KevinMultimodalClassifier("concatenation", text=tc, image=ic, caption=_golden_cfg(pkg, golden), proj=64,
                                          compute_dtype="fp16", seed=3)
    model.cuda().train()
    g = torch.Generator().manual_seed(9)
    text = torch.randint(5, 300, (B, S), generator=g)
    tmask = (torch.arange(S)[None] < torch.tensor([16, 9, 12, 5])[:, None]).long()
    cap, image, labels = _batch(B, S, ["right", "none", "interior", "right"], 10)
    cmask = (cap != 1).long()
    groups = model.get_params(1.0)
    table = model.caption_text_model.inner._params[POS]
    assert table.shape == (24, 128)
    where = [gi for gi, gr in enumerate(groups) if any(p is table for p in gr["params"])]
    assert where == [1] and groups[1]["lr"] == 0.8
    out = model(text.cuda() * tmask.cuda(), image.cuda(), tmask.cuda(), cap.cuda(), cmask.cuda())
    loss = pkg.SigmoidFocalLoss()(out, labels.float().cuda(), alpha=0.25, gamma=2.0, reduction="mean")
    loss.backward()
    torch.cuda.synchronize()
    assert out.shape == (B,) and np.isfinite(float(loss.detach()))
    gpos = table.grad
    assert bool(torch.isfinite(gpos).all()) and float(gpos[2:18].abs().sum()) > 0
    assert bool((gpos[:2] == 0).all()) and bool((gpos[18:] == 0).all()), "row pad_id (or a row no token reads) received a gradient"
