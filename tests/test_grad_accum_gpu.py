"""Gradient accumulation over micro-batches for the transformer towers (``set_grad_accumulation``), on the MI355X.

With the switch on, a backward overwrites the gradients when they were cleared since the previous backward and adds otherwise.
What is asserted, and why it can be asserted bit for bit:

  * the first backward of a window is the overwriting backward, launch for launch: the same bits as with the switch off;
  * an adding backward computes the micro-batch's own gradient exactly as the overwriting one stores it -- the same kernels over
    the same operands, rounded to f32 once -- and then adds it to what ``.grad`` holds in ONE f32 add per element: in the epilogue
    of the weight-gradient GEMMs (``alpha`` is 1 or 2^-13, a power of two, so a contracted multiply-add rounds like multiply then
    add), in ``mh_bert_embed_bwd_accum`` (product and sum rounded separately) and in ``mh_accum_spans_f32`` for everything else.
    So ``.grad`` after a window of three micro-batches is ``((g_1 + g_2) + g_3)`` as torch computes it in f32 from the three
    gradients taken alone.  No path of the towers is held to anything weaker.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LR = 2e-5


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import multimodal_propaganda_meme_classification_amd as m
    return m


def _oracle():
    from oracle import meme_oracle as O
    return O


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------------------
# the two new entry points on their own
# ---------------------------------------------------------------------------------------------------------------------------
def test_accum_spans_adds_every_element_once(pkg):
    """mh_accum_spans_f32: dst += src over several spans of one launch -- sizes around the 4096-element workgroup tile and the
    16-byte vector (1, 3, 4, 5, 4095, 4096, 4097, 3 tiles + 2), MH_SPAN_MAX_JOBS spans at once; one f32 add per element (equal to
    torch's, bit for bit), nothing written outside a span (guard elements on both sides), refusals for misaligned / empty spans."""
    lib = pkg._lib.load()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(11)
    sizes = [1, 3, 4, 5, 4095, 4096, 4097, 3 * 4096 + 2, 8, 12, 260, 1023, 1024, 1025, 7, 64]
    assert len(sizes) == pkg._lib.MH_SPAN_MAX_JOBS
    GUARD = 8
    dsts, srcs, want = [], [], []
    for n in sizes:
        pad = (n + 3) // 4 * 4
        d = torch.randn(GUARD + pad + GUARD, generator=g).cuda()
        s = (torch.randn(pad, generator=g) * 3).cuda()
        w = d.clone()
        w[GUARD:GUARD + n] += s[:n]
        dsts.append(d), srcs.append(s), want.append(w)
    arr = (pkg._lib.MhSpanJob * len(sizes))()
    for e, d, s, n in zip(arr, dsts, srcs, sizes):
        e.dst, e.src, e.n = d.data_ptr() + 4 * GUARD, s.data_ptr(), n
    assert lib.mh_accum_spans_f32(arr, len(sizes), st) == 0
    torch.cuda.synchronize()
    for d, w, n in zip(dsts, want, sizes):
        assert _same_bits(d, w), n
    one = (pkg._lib.MhSpanJob * 1)()
    one[0].dst, one[0].src, one[0].n = dsts[0].data_ptr() + 4, srcs[0].data_ptr(), 1       # dst not 16-byte aligned
    assert lib.mh_accum_spans_f32(one, 1, st) != 0
    one[0].dst, one[0].n = dsts[0].data_ptr() + 4 * GUARD, 0                                 # empty span
    assert lib.mh_accum_spans_f32(one, 1, st) != 0
    assert lib.mh_accum_spans_f32(arr, pkg._lib.MH_SPAN_MAX_JOBS + 1, st) != 0
    assert lib.mh_accum_spans_f32(None, 1, st) != 0


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("indexed", [True, False], ids=["indexed", "plain"])
def test_embed_bwd_accum_adds_what_embed_bwd_stores(pkg, kind, indexed):
    """mh_bert_embed_bwd_accum against mh_bert_embed_bwd on the same ids and d_pre: every touched row of dword ends as
    old + (what mh_bert_embed_bwd stores), one f32 add, bit for bit; untouched rows and the pad row keep their old value; dpos and
    dtype0 are overwritten with mh_bert_embed_bwd's bits.  Duplicated ids (first-occurrence owner), ids out of range (ignored),
    D = 128 and 640 (one and two column chunks of 512, the second ragged), scale 2^-13 and 0.37 (not a power of two: product and sum must
    be rounded separately)."""
    lib = pkg._lib.load(kind)
    T16 = torch.float16 if kind == "fp16" else torch.bfloat16
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(5)
    V, pad_id = 40, 0
    for (B, S, D, scale) in ((3, 7, 128, 2.0 ** -13), (2, 5, 640, 0.37), (5, 9, 128, 1.0)):
        ids = torch.randint(0, 12, (B, S), generator=g)
        ids[0, 0] = V + 3                      # out of range: ignored
        ids[B - 1, S - 1] = -1
        d_pre = torch.randn(B * S, D, generator=g).to(T16).cuda()
        ids_d = ids.cuda()
        old = torch.randn(V, D, generator=g).cuda()
        base, acc = torch.zeros(V, D).cuda(), old.clone()
        pos_b, pos_a = torch.zeros(S, D).cuda(), torch.full((S, D), 7.0).cuda()
        ty_b, ty_a = torch.zeros(D).cuda(), torch.full((D,), 7.0).cuda()
        live = torch.zeros(V, dtype=torch.uint8).cuda()
        first = torch.full((V,), 0x7fffffff, dtype=torch.int32).cuda()
        count = torch.zeros(V, dtype=torch.int32).cuda()
        idx = (first.data_ptr(), count.data_ptr()) if indexed else (None, None)
        args = (B, S, D, V, pad_id, scale, live.data_ptr(), idx[0], idx[1], st)
        assert lib.mh_bert_embed_bwd(ids_d.data_ptr(), d_pre.data_ptr(), base.data_ptr(), pos_b.data_ptr(), ty_b.data_ptr(), *args) == 0
        assert lib.mh_bert_embed_bwd_accum(ids_d.data_ptr(), d_pre.data_ptr(), acc.data_ptr(), pos_a.data_ptr(), ty_a.data_ptr(), *args) == 0
        torch.cuda.synchronize()
        touched = torch.zeros(V, dtype=torch.bool)
        ok = ids[(ids > 0) & (ids < V)]
        touched[ok] = True
        assert not bool(touched[pad_id]) and int(touched.sum()) >= 5
        want = torch.where(touched.cuda()[:, None], old + base, old)
        assert _same_bits(acc, want), (B, S, D, scale)
        assert float(base[~touched.cuda()].abs().max()) == 0.0
        assert _same_bits(pos_a, pos_b) and _same_bits(ty_a, ty_b)
        if indexed:
            assert int((first != 0x7fffffff).sum()) == 0 and int(count.abs().sum()) == 0       # the index restores itself


# ---------------------------------------------------------------------------------------------------------------------------
# models and micro-batches
# ---------------------------------------------------------------------------------------------------------------------------
def _tiny_dict(O, pool="cls"):
    return O.tiny_config(pool).to_dict()


def _cases(pkg):
    """name -> (ModelConfig dict, features, micro-batch shapes)"""
    O = _oracle()
    win = ((3, 12), (2, 8), (3, 12))
    out = {}
    d = _tiny_dict(O, "cls")
    out["tiny-cls-bf16-packed"] = (d, False, win)
    d = _tiny_dict(O, "last")
    d["compute_dtype"] = "fp16"
    out["tiny-last-fp16-packed"] = (d, False, win)
    d = _tiny_dict(O, "cls")
    d["text"]["layers"] = 3
    d["pack_text"] = False
    out["text3-image2-dense"] = (d, False, win)
    d = _tiny_dict(O, "last")
    d["compute_dtype"] = "fp16"
    out["features-pooled-fp16"] = (d, True, win)
    d = _tiny_dict(O, "cls")
    out["features-sequence-bf16"] = (d, "sequence", win)
    d = _tiny_dict(O, "cls")
    d["text"] = pkg.TextConfig.roberta_base(vocab_size=64, max_position=40, hidden=128, layers=2, heads=2, intermediate=256).__dict__.copy()
    out["roberta-text"] = (d, False, win)
    d = _tiny_dict(O, "cls")
    d["compute_dtype"] = "fp16"
    d["image"].update(image_size=28, patch=14, act="quick_gelu", pre_ln=True, patch_bias=False, ln_eps=1e-5)
    out["clip-image-padded-k"] = (d, False, win)
    d = _tiny_dict(O, "cls")
    d["image"].update(image_size=512, patch=16, layers=1)
    out["patch-split-k"] = (d, False, ((1, 12), (1, 8), (1, 12)))
    return out


CASE_NAMES = ["tiny-cls-bf16-packed", "tiny-last-fp16-packed", "text3-image2-dense", "features-pooled-fp16", "features-sequence-bf16",
              "roberta-text", "clip-image-padded-k", "patch-split-k"]


def _model(pkg, d, seed=7):
    cfg = pkg.ModelConfig.from_dict(d)
    m = pkg.MultimodalClassifier.from_config(cfg, seed=seed)
    with torch.no_grad():       # biases and LayerNorm parameters away from their 0 / 1 initial values
        gen = torch.Generator().manual_seed(seed + 1)
        for n, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=gen) * 0.05)
    m.mark_weights_changed()
    return m.to("cuda").train()


def _micro_batch(cfg, B, S, seed):
    """Ragged masks with a sequence of length 1 whenever B > 1; padded positions hold the pad id."""
    g = torch.Generator().manual_seed(seed)
    t, v = cfg.text, cfg.image
    ids = torch.randint(5, t.vocab_size, (B, S), generator=g)
    lens = torch.randint(2, S + 1, (B,), generator=g)
    lens[0] = S
    if B > 1:
        lens[1] = 1
    mask = (torch.arange(S)[None] < lens[:, None]).long()
    ids[:, 0] = 2
    ids = torch.where(mask.bool(), ids, torch.full_like(ids, t.pad_token_id))
    image = torch.randn((B, v.channels, v.image_size, v.image_size), generator=g)
    labels = torch.randint(0, cfg.num_classes, (B,), generator=g)
    w_t, w_i = torch.randn((B, S, t.hidden), generator=g), torch.randn((B, v.n_tokens, v.hidden), generator=g)
    return [x.cuda() for x in (ids, image, mask, labels, w_t, w_i)]


FEATURE_GRAD = 1e-2     # size of d loss / d feature in the features modes: the fp16 build's 16-bit gradient streams carry 8192 times
                        # the gradient, so a gradient of order 1 per element (a head would hand over ~1 / batch) overflows them


def _loss(model, crit, features, mb, weight=1.0):
    ids, image, mask, labels, w_t, w_i = mb
    if features == "sequence":
        h_t, h_i = model.encode_sequence(ids, image, mask)
        return ((h_t * w_t).sum() + (h_i * w_i).sum()) * (weight * FEATURE_GRAD)
    if features:
        f_t, f_i = model.encode(ids, image, mask)
        return ((f_t * w_t[:, 0]).sum() + (f_i * w_i[:, 0]).sum()) * (weight * FEATURE_GRAD)
    return crit(model(ids, image, mask), labels) * weight


def _alone(model, crit, features, mb, weight=1.0):
    """The micro-batch's gradient with the switch off, from a zeroed buffer: the whole flat buffer.  (A step's gradient does not
    depend on what the buffer held, tests/test_history_independence_gpu.py; the zeroing only keeps this helper self-contained.)"""
    was = model.grad_accumulation
    model.set_grad_accumulation(False)
    model.flat_grads.zero_()
    _loss(model, crit, features, mb, weight).backward()
    torch.cuda.synchronize()
    model.set_grad_accumulation(was)
    return model.flat_grads.clone()


def _report(model, got, want):
    """names of the parameters whose gradient differs in some bit, with the count"""
    bad = []
    for name, s in model.layout.spec.items():
        a, b = got[s.offset:s.offset + s.numel], want[s.offset:s.offset + s.numel]
        n = int((_bits(a) != _bits(b)).sum())
        if n:
            bad.append((name, n, float((a - b).abs().max())))
    return bad


@pytest.mark.parametrize("case", CASE_NAMES)
def test_window_gradient_is_the_f32_sum_bit_for_bit(pkg, case):
    """Sum rule: .grad after a window of three micro-batches (B = 3, 2, 3; S = 12, 8, 12: two plans, a plan switch inside the window)
    equals ((g_1 + g_2) + g_3) in f32, every parameter, every bit."""
    d, features, shapes = _cases(pkg)[case]
    model = _model(pkg, d)
    crit = pkg.CrossEntropyLoss()
    mbs = [_micro_batch(model.config, B, S, seed=100 + k) for k, (B, S) in enumerate(shapes)]
    alone = [_alone(model, crit, features, mb, weight=1.0 / 3) for mb in mbs]
    assert all(bool(torch.isfinite(a).all()) and float(a.abs().sum()) > 0 for a in alone)
    want = (alone[0] + alone[1]) + alone[2]
    model.set_grad_accumulation(True)
    assert model.grad_accumulation
    # a window before the one that is checked: its rows and sums must not leak into the next one
    opt = pkg.Adam(model.parameters(), lr=LR)
    for window in range(2):
        opt.zero_grad()
        for mb in (mbs if window else mbs[::-1]):
            _loss(model, crit, features, mb, weight=1.0 / 3).backward()
    torch.cuda.synchronize()
    got = model.flat_grads
    bad = _report(model, got, want)
    print(case, "parameters with a differing bit:", bad)
    assert not bad, bad
    assert _same_bits(got, want)
    for n, p in model.named_parameters():           # the views autograd users read are views of that buffer
        s = model.layout.spec["image_fc" + n[len(model.config.image_fc_name):] if n.startswith(model.config.image_fc_name + ".") else n]
        assert p.grad.data_ptr() == got.data_ptr() + 4 * s.offset


def test_sum_rule_fails_without_the_switch(pkg):
    """The trap the switch closes: with it off, the same window leaves the last micro-batch's gradient alone."""
    d, features, shapes = _cases(pkg)["tiny-cls-bf16-packed"]
    model = _model(pkg, d)
    crit = pkg.CrossEntropyLoss()
    mbs = [_micro_batch(model.config, B, S, seed=100 + k) for k, (B, S) in enumerate(shapes)]
    alone = [_alone(model, crit, features, mb) for mb in mbs]
    model.flat_grads.zero_()
    for mb in mbs:
        _loss(model, crit, features, mb).backward()
    torch.cuda.synchronize()
    name = "bert.encoder.layer.0.output.dense.weight"
    s = model.layout.spec[name]
    sl = slice(s.offset, s.offset + s.numel)
    assert _same_bits(model.flat_grads[sl], alone[2][sl])
    assert not torch.equal(model.flat_grads[sl], ((alone[0] + alone[1]) + alone[2])[sl])


@pytest.mark.parametrize("route", ["adam_zero_grad", "parent_zero_grad", "parent_zero_grad_in_place"])
def test_first_micro_batch_of_a_window_equals_the_overwriting_backward(pkg, route):
    """Switch on, ONE micro-batch after the gradients were cleared: bit-identical to the switch-off gradient, for the three ways of
    clearing -- memehip.Adam.zero_grad(), nn.Module.zero_grad() on a parent composite (.grad becomes None: detected at the backward)
    and zero_grad(set_to_none=False) on it (zeroed in place: the backward ADDS to zeros)."""
    d, features, shapes = _cases(pkg)["tiny-last-fp16-packed"]
    model = _model(pkg, d)
    parent = pkg.TrainerModel(model)
    crit = pkg.CrossEntropyLoss()
    mbs = [_micro_batch(model.config, B, S, seed=200 + k) for k, (B, S) in enumerate(shapes)]
    want = _alone(model, crit, features, mbs[1])
    parent.set_grad_accumulation(True)
    assert model.grad_accumulation and parent.grad_accumulation
    opt = pkg.Adam(model.parameters(), lr=LR)
    opt.zero_grad()
    for mb in (mbs[0], mbs[2]):                      # a window of two, so that there is something to clear
        _loss(model, crit, features, mb).backward()
    if route == "adam_zero_grad":
        opt.zero_grad()
    elif route == "parent_zero_grad":
        parent.zero_grad()
        assert all(p.grad is None for p in model.parameters())
    else:
        parent.zero_grad(set_to_none=False)
        assert float(model.flat_grads.abs().max()) == 0.0
    _loss(model, crit, features, mbs[1]).backward()
    torch.cuda.synchronize()
    bad = _report(model, model.flat_grads, want)
    print(route, "parameters with a differing bit:", bad)
    assert not bad, bad
    assert all(p.grad is not None for p in model.parameters())


def _grad_check(model, grads, rel=3e-2):
    """tests/test_model_gpu.py::_grad_check, restated: per parameter ||hip - oracle|| <= 3e-2 ||oracle|| + 2e-6; the analytically zero
    key bias below 1e-4."""
    for name, p in model.named_parameters():
        ref = grads[name]
        got = p.grad.detach().float().cpu()
        num, den = float((got - ref).norm()), float(ref.norm())
        if ".key.bias" in name:
            assert num < 1e-4, (name, num)
            continue
        assert num <= rel * den + 2e-6, f"grad {name}: ||diff||={num:.3e} ||ref||={den:.3e}"


def test_two_half_batches_match_the_oracle_on_the_whole_batch(pkg, golden_dir):
    """Two half-batches with loss / 2 against oracle.meme_oracle.train_step on the whole batch: gradients within the per-parameter
    bound of tests/test_model_gpu.py for this config, then one Adam.step() against the oracle's in
    test_tiny_step_matches_oracle_and_golden's form (every element within 2.05 lr, mean deviation below 0.05 lr).  The batch and the
    parameters are that test's own (tests/golden/tiny_cls.npz), on which its bound was set: the bound is relative to the gradient's
    norm, and on a batch with small gradients the single-batch path itself is outside it (synthetic_batch(seed=31), mixed labels:
    7.6e-2 for the whole batch in one backward, the same 7.6e-2 for its two halves accumulated)."""
    O = _oracle()
    z = np.load(os.path.join(golden_dir, "tiny_cls.npz"))
    cfg = O.tiny_config("cls")
    params = O.init_params(cfg, int(z["seed"]))
    model = pkg.MultimodalClassifier.from_config(pkg.ModelConfig.from_dict(cfg.to_dict()), init=False)
    model.load_state_dict(params)
    model.to("cuda").train()
    model.set_grad_accumulation(True)
    text, image, mask, labels = (torch.from_numpy(z[k]) for k in ("text", "image", "mask", "labels"))
    st = O.AdamState()
    p_ref, _, ref_loss, ref_grads = O.train_step(params, st, text, image, mask, labels, cfg, lr=LR)
    opt = pkg.Adam(model.parameters(), lr=LR)
    crit = pkg.CrossEntropyLoss()
    opt.zero_grad()
    total = 0.0
    for half in (slice(0, 2), slice(2, 4)):
        loss = crit(model(text[half].cuda(), image[half].cuda(), mask[half].cuda()), labels[half].cuda()) / 2
        loss.backward()
        total += float(loss.detach())
    assert abs(total - float(ref_loss)) <= 3e-3
    _grad_check(model, ref_grads)
    opt.step()
    torch.cuda.synchronize()
    sd = model.state_dict()
    tot, cnt = 0.0, 0
    for k, ref in p_ref.items():
        dlt = (sd[k].detach().float().cpu() - ref).abs()
        assert float(dlt.max()) <= 2.05 * LR, (k, float(dlt.max()))
        if ".key.bias" not in k:
            tot += float(dlt.sum())
            cnt += dlt.numel()
    assert tot / cnt < 0.05 * LR, tot / cnt


def test_word_table_rows_add_inside_a_window_and_clear_between_windows(pkg):
    """Vocabulary 64.  Window 1 touches ids {1, 2, 3}, then {3, 4}: row 3 holds the f32 sum, rows 1, 2 and 4 their micro-batch's
    own gradient.  Window 2 touches {5} only, under another (B, S): rows 1-4 are exactly zero after it.  The pad row is zero
    throughout.  A third window with a shorter sequence: the position-table rows past it are zero again."""
    O = _oracle()
    d = _tiny_dict(O, "cls")
    d["text"]["vocab_size"] = 64
    model = _model(pkg, d)
    crit = pkg.CrossEntropyLoss()
    g = torch.Generator().manual_seed(3)

    def mb(rows, S):
        ids = torch.tensor(rows)
        B = ids.shape[0]
        return [x.cuda() for x in (ids, torch.randn((B, 3, 32, 32), generator=g), (ids != 0).long(), torch.randint(0, 2, (B,), generator=g))] + [None, None]

    a = mb([[1, 2, 3, 0], [2, 1, 0, 0]], 4)
    b = mb([[3, 4, 4, 0], [4, 3, 3, 3]], 4)
    c = mb([[5, 5, 5, 0, 0, 0]], 6)
    e = mb([[6, 7, 0]], 3)
    word = model.layout.spec["bert.embeddings.word_embeddings.weight"]
    pos = model.layout.spec["bert.embeddings.position_embeddings.weight"]
    D = model.config.text.hidden

    def rows(flat, spec=word):
        return flat[spec.offset:spec.offset + spec.numel].view(-1, D)

    ga, gb = rows(_alone(model, crit, False, a)).clone(), rows(_alone(model, crit, False, b)).clone()
    model.set_grad_accumulation(True)
    opt = pkg.Adam(model.parameters(), lr=LR)
    opt.zero_grad()
    _loss(model, crit, False, a).backward()
    _loss(model, crit, False, b).backward()
    torch.cuda.synchronize()
    got = rows(model.flat_grads)
    assert float(ga[3].abs().sum()) > 0 and float(gb[3].abs().sum()) > 0
    assert _same_bits(got[3], ga[3] + gb[3])
    assert _same_bits(got[1], ga[1]) and _same_bits(got[2], ga[2]) and _same_bits(got[4], gb[4])
    assert float(got[0].abs().max()) == 0.0 and float(got[5:].abs().max()) == 0.0
    opt.zero_grad()
    _loss(model, crit, False, c).backward()
    torch.cuda.synchronize()
    got = rows(model.flat_grads)
    assert float(got[1:5].abs().max()) == 0.0, "rows of the previous window survive"
    assert float(got[5].abs().sum()) > 0 and float(got[0].abs().max()) == 0.0 and float(got[6:].abs().max()) == 0.0
    assert float(rows(model.flat_grads, pos)[:6].abs().sum()) > 0
    opt.zero_grad()
    _loss(model, crit, False, e).backward()
    torch.cuda.synchronize()
    got = rows(model.flat_grads)
    assert float(got[:6].abs().max()) == 0.0 and float(got[6].abs().sum()) > 0 and float(got[7].abs().sum()) > 0
    gp = rows(model.flat_grads, pos)
    assert float(gp[3:].abs().max()) == 0.0 and float(gp[:3].abs().sum()) > 0


def test_overflow_in_the_middle_of_a_window_skips_the_whole_step_once(pkg):
    """fp16 + GradScaler: an inf pixel in the MIDDLE micro-batch of a window (as tests/test_scaler_gpu.py injects one).  The
    non-finite values added into .grad stay non-finite, the step-time check sees them: parameters, moments and the 16-bit shadow are
    unchanged, the step is counted once, the scale backs off once; the next clean window updates."""
    d, features, shapes = _cases(pkg)["tiny-last-fp16-packed"]
    model = _model(pkg, d)
    model.set_grad_accumulation(True)
    crit = pkg.CrossEntropyLoss()
    opt = pkg.Adam(model.parameters(), lr=1e-3)
    scaler = pkg.GradScaler()
    scales, skipped = [], []
    for window, kind in enumerate(("ok", "overflow", "ok")):
        mbs = [_micro_batch(model.config, B, S, seed=300 + 10 * window + k) for k, (B, S) in enumerate(shapes)]
        if kind == "overflow":
            mbs[1][1][1, 0, 3, 3] = float("inf")
        before = (model.flat_params.clone(), model.flat_shadow.clone(), opt._flat["M"].clone() if opt._flat else None,
                  opt._flat["V"].clone() if opt._flat else None)
        opt.zero_grad()
        for mb in mbs:
            scaler.scale(_loss(model, crit, features, mb, weight=1.0 / 3)).backward()
        scaler.step(opt)
        scaler.update()
        torch.cuda.synchronize()
        scales.append(scaler.get_scale())
        skipped.append(opt.skipped_steps)
        if kind == "overflow":
            assert not bool(torch.isfinite(model.flat_grads).all())
            assert torch.equal(model.flat_params, before[0]) and torch.equal(model.flat_shadow, before[1])
            assert torch.equal(opt._flat["M"], before[2]) and torch.equal(opt._flat["V"], before[3])
            assert opt.last_step_skipped
        else:
            assert bool(torch.isfinite(model.flat_grads).all()) and bool(torch.isfinite(model.flat_params).all())
            assert not torch.equal(model.flat_params, before[0]) and not opt.last_step_skipped
    assert scales == [1.0, 0.5, 0.5] and skipped == [0, 1, 1], (scales, skipped)


def test_hf_trainer_with_gradient_accumulation_steps(pkg, tmp_path):
    """transformers.Trainer(gradient_accumulation_steps=2) on a tiny TextClassifier for two optimizer steps, against the same four
    micro-batches driven by hand (AdamW, linear schedule, clip 1.0, model.zero_grad(): Trainer's own sequence): bit-identical
    parameters.  Against the same run with the switch off they differ: there each step used its last micro-batch alone."""
    pytest.importorskip("transformers")
    pytest.importorskip("accelerate")
    from transformers import Trainer, TrainingArguments, default_data_collator, get_scheduler
    B, S, N, steps, lr = 3, 12, 2, 2, 1e-3
    tc = pkg.TextConfig(vocab_size=200, hidden=128, layers=2, heads=2, intermediate=256, max_position=32, type_vocab=0)
    g = torch.Generator().manual_seed(9)
    n = B * N * steps
    ids = torch.randint(5, 200, (n, S), generator=g)
    lens = torch.randint(1, S + 1, (n,), generator=g)
    mask = (torch.arange(S)[None] < lens[:, None]).long()
    ids = ids * mask
    labels = torch.randint(0, 2, (n,), generator=g)

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return n

        def __getitem__(self, i):
            return {"input_ids": ids[i], "attention_mask": mask[i], "labels": int(labels[i])}

    class InOrder(Trainer):
        def _get_train_sampler(self, *a, **k):
            return torch.utils.data.SequentialSampler(self.train_dataset)

    def make():
        torch.manual_seed(0)
        return pkg.TextClassifier(tc, pooling_type="mean", num_classes=2, compute_dtype="bf16", seed=4)

    m_tr = make()
    init = {k: v.detach().clone() for k, v in m_tr.state_dict().items()}
    m_tr.set_grad_accumulation(True)
    args = TrainingArguments(output_dir=str(tmp_path), learning_rate=lr, num_train_epochs=1, per_device_train_batch_size=B,
                             gradient_accumulation_steps=N, save_strategy="no", report_to=[], logging_steps=1, seed=42,
                             remove_unused_columns=False, optim="adamw_torch", weight_decay=0.0, lr_scheduler_type="linear",
                             warmup_steps=0, max_grad_norm=1.0, dataloader_drop_last=False)
    trainer = InOrder(model=m_tr, args=args, train_dataset=DS(), data_collator=default_data_collator)
    trainer.model_accepts_loss_kwargs = False          # forward(**unused) ignores num_items_in_batch: Trainer divides the loss by N itself
    res = trainer.train()
    assert trainer.state.global_step == steps and np.isfinite(res.training_loss)

    def by_hand(switch):
        m = make().cuda().train()
        m.load_state_dict(init)
        m.set_grad_accumulation(switch)
        opt = torch.optim.AdamW(m.parameters(), lr=lr, betas=(args.adam_beta1, args.adam_beta2), eps=args.adam_epsilon, weight_decay=0.0)
        sched = get_scheduler("linear", opt, num_warmup_steps=0, num_training_steps=steps)
        m.zero_grad()
        for k in range(N * steps):
            sl = slice(k * B, (k + 1) * B)
            loss, _ = m(input_ids=ids[sl].cuda(), attention_mask=mask[sl].cuda(), labels=labels[sl].cuda())
            (loss / N).backward()
            if (k + 1) % N == 0:
                torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
                opt.step()
                sched.step()
                m.zero_grad()
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in m.state_dict().items()}

    on, off = by_hand(True), by_hand(False)
    got = m_tr.state_dict()
    bad = [k for k in on if not torch.equal(got[k].detach(), on[k])]
    print("Trainer vs by hand, parameters that differ:", bad)
    assert not bad, bad
    assert any(not torch.equal(on[k], off[k]) for k in on)
    assert any(not torch.equal(on[k].cpu(), init[k].cpu()) for k in on)


def test_kevins_model_follows_the_sum_rule_in_every_part(pkg):
    """KevinMultimodalClassifier(image="resnet18"): two micro-batches with the switch on against the two taken alone.  Text and
    caption towers: bit for bit (the paths of the sum-rule test).  The flattened head receives its gradient from autograd, which adds
    with one f32 add: bit for bit as well.  The ResNet tower adds inside its own kernels (split-K finishers, BatchNorm partials):
    held to the bound tests/test_basic_resnet_gpu.py sets for that tower's in-place accumulation, |diff| <= 1e-6 max|ref| + 1e-12.
    The global gradient norm (what tests/test_heads_gpu.py checks against its oracle, 3 %) agrees with the norm of the sum."""
    tc = pkg.TextConfig(vocab_size=600, hidden=128, layers=2, heads=2, intermediate=256, max_position=64)
    cc = pkg.TextConfig(vocab_size=500, hidden=128, layers=1, heads=2, intermediate=256, max_position=64)
    model = pkg.KevinMultimodalClassifier("concatenation", text=tc, image="resnet18", caption=cc, proj=128, compute_dtype="bf16", seed=1,
                                          resnet_layers=(1, 1, 1, 1))
    model.text_dropout.p = model.caption_text_dropout.p = 0.0
    model.image_fine_tune[2].p = 0.0
    model.cuda().train()
    opt = pkg.Adam(model.get_params(1e-4), lr=1e-4, max_grad_norm=1.0)
    crit = pkg.SigmoidFocalLoss()
    g = torch.Generator().manual_seed(5)

    def mb(B, S):
        text, cap = torch.randint(5, 600, (B, S), generator=g), torch.randint(5, 500, (B, S), generator=g)
        lens = torch.randint(1, S + 1, (B,), generator=g)
        mask = (torch.arange(S)[None] < lens[:, None]).long()
        image = torch.randn((B, 3, 64, 64), generator=g)
        labels = (torch.rand(B, generator=g) < 0.4).float()
        return [x.cuda() for x in (text * mask, image, mask, cap * mask, mask)], labels.cuda()

    mbs = [mb(4, 12), mb(3, 8)]

    def backward(batch):
        x, y = batch
        (crit(model(*x), y, alpha=0.25, gamma=2.0, reduction="mean") / 2).backward()

    def grads():
        torch.cuda.synchronize()
        return {n: p.grad.detach().clone() for n, p in model.named_parameters()}

    alone = []
    for batch in mbs:
        opt.zero_grad()
        model.text_model.inner.flat_grads.zero_(), model.caption_text_model.inner.flat_grads.zero_()
        backward(batch)
        alone.append(grads())
    model.set_grad_accumulation(True)
    assert model.grad_accumulation and model.text_model.grad_accumulation and model.caption_text_model.grad_accumulation
    opt.zero_grad()
    for batch in mbs:
        backward(batch)
    got = grads()
    bad = []
    for n, gsum in got.items():
        want = alone[0][n] + alone[1][n]
        if n.startswith("image_model."):
            ok = float((gsum - want).abs().max()) <= 1e-6 * float(want.abs().max()) + 1e-12
        else:
            ok = _same_bits(gsum, want)
        if not ok:
            bad.append((n, float((gsum - want).abs().max()), float(want.abs().max())))
    print("Kevin's model, parameters off the sum rule:", bad)
    assert not bad, bad
    assert sum(float(v.abs().sum()) > 0 for v in got.values()) > 40
    ref_norm = float(torch.sqrt(sum(((alone[0][n] + alone[1][n]).double() ** 2).sum() for n in got)))
    norm = float(opt.grad_norm())
    assert abs(norm - ref_norm) < 0.03 * ref_norm + 1e-6, (norm, ref_norm)


def test_a_dropped_model_frees_its_plans_without_the_cyclic_collector(pkg):
    """A plan owns every activation of its shape (gigabytes at the benchmarked sizes) and has to die with its model by reference
    count: with the adding flavour built as well, dropping the model returns the device memory while gc is disabled."""
    import gc
    import weakref
    d, features, shapes = _cases(pkg)["tiny-cls-bf16-packed"]
    crit = pkg.CrossEntropyLoss()
    torch.cuda.synchronize()
    gc.collect()
    base = None
    gc.disable()
    try:
        for switch in (False, False, True):       # (the first round only warms whatever the library allocates once per process)
            model = _model(pkg, d)
            model.set_grad_accumulation(switch)
            mbs = [_micro_batch(model.config, B, S, seed=400 + k) for k, (B, S) in enumerate(shapes[:2])]
            for mb in mbs + mbs:
                _loss(model, crit, features, mb).backward()
            torch.cuda.synchronize()
            eng = model._get_engine()
            plans = [weakref.ref(p) for p in eng.plans.values()]
            assert len(plans) == 2 and all((p().bwd_add is not None) == switch for p in plans)
            ref_eng = weakref.ref(eng)
            assert base is None or torch.cuda.memory_allocated() > base
            del model, eng, mbs, mb
            assert ref_eng() is None and all(p() is None for p in plans), switch
            if base is None:
                base = torch.cuda.memory_allocated()
            assert torch.cuda.memory_allocated() == base, (switch, torch.cuda.memory_allocated(), base)
    finally:
        gc.enable()


def test_refusals(pkg):
    """With the switch on: GraphedStep, forward_backward and a reducer hook raise ValueError naming the switch; a second forward of a
    shape before its backward still raises the generation error, whose text now points at set_grad_accumulation."""
    d, features, shapes = _cases(pkg)["tiny-cls-bf16-packed"]
    model = _model(pkg, d)
    crit = pkg.CrossEntropyLoss()
    opt = pkg.Adam(model.parameters(), lr=LR)
    ids, image, mask, labels, _, _ = _micro_batch(model.config, 3, 12, seed=1)
    model.set_grad_accumulation(True)
    with pytest.raises(ValueError, match="set_grad_accumulation"):
        pkg.GraphedStep(model, opt, 3, 12)
    with pytest.raises(ValueError, match="autograd path"):
        model.forward_backward(ids, image, mask, labels)
    seen = []
    with pytest.raises(ValueError, match="reducer hooks"):
        model.forward_backward(ids, image, mask, labels, grad_hook=lambda name, rng: seen.append(name))
    assert not seen
    first = model(ids, image, mask)
    second = model(ids, image, mask)
    crit(second, labels).backward()
    with pytest.raises(RuntimeError, match="overwritten by a later forward") as err:
        crit(first, labels).backward()
    assert "set_grad_accumulation" in str(err.value)
    # a step built before the switch was turned on refuses at step()
    model.set_grad_accumulation(False)
    gs = pkg.GraphedStep(model, opt, 3, 12, use_graph=False)
    model.set_grad_accumulation(True)
    with pytest.raises(ValueError, match="set_grad_accumulation"):
        gs.step()
    gs.close()
    # the switch is a runtime property: the config and its dict form do not know it
    assert "grad_accumulation" not in str(model.config.to_dict())
    enc = pkg.TextEncoder(pkg.TextConfig(vocab_size=64, hidden=128, layers=1, heads=2, intermediate=128, max_position=16))
    assert enc.set_grad_accumulation(True) is enc and enc.grad_accumulation and enc.inner.grad_accumulation
    assert not enc.set_grad_accumulation(False).grad_accumulation
