"""No step's outputs or gradients depend on what the model object ran before, on the MI355X.

The transformer engine keeps state from one batch to the next: one launch plan per shape with its activations, split-K workspaces,
packed-row maps and device-side row counts; the dense word-table gradient, re-zeroed only on the rows of the previous ids; the
self-restoring id index; ``word_row_live``; the scratch mirror of the small gradients; the position-row bookkeeping; the compact last
layer's scatter-with-zero-fill; the head's gradient slots on the ``encode`` paths.  The per-kernel tests run on fresh buffers and
cannot see a mistake in any of it.  The property held here needs no tolerance:

    the outputs and gradients of a step are a function of the weights, the batch and the dropout seed -- never of what the model
    object ran earlier.

Twin protocol: two models from the same parameters (tests/test_grad_accum_gpu._model: 1-D parameters nudged away from 0 / 1).
*Fresh* runs only the probe; *used* first runs a history through the public entry points (no optimizer step: the weights stay equal),
then the same probe.  Compared on int32 views, every bit: the probe's outputs (logits, loss, correct count, features), the whole flat
gradient buffer with its alignment padding, every parameter's ``.grad``, and, after one ``memehip.Adam`` step created after the
history, the master weights, the 16-bit shadow and both moment buffers.  Facts that do not rest on the twin are asserted on the used
model alone as exact zeros: position-table gradient rows >= S (absolute scheme), word-table rows of ids outside the probe and the pad
row, token-type rows >= 1, and every built-in head parameter's gradient on the ``encode`` / ``encode_sequence`` paths.

Against a vacuous pass: the history's last gradient differs from the probe's, the history touched >= 5 word rows the probe does not,
the probe's gradient is finite and non-zero for every parameter outside the zero list (the attention key biases, whose gradient is
analytically zero -- a softmax row's gradient sums to zero -- and numerically rounding noise, need only be finite), and the poisoned
history really left non-finite values behind.  Every guard quantity goes through conftest.parity_log.
"""
import pytest
import torch

from conftest import parity_log
from test_grad_accum_gpu import CASE_NAMES, FEATURE_GRAD, _cases, _model, _report

pytestmark = pytest.mark.gpu

LR = 2e-5
SEED = 77
CONFIGS = CASE_NAMES + ["reference-dropout-bf16"]
HEAD = ("bert_fc.", "image_fc.", "resnet_fc.", "fusion_fc.", "output_fc.")
WORD = "bert.embeddings.word_embeddings.weight"
POS = "bert.embeddings.position_embeddings.weight"
TYPE = "bert.embeddings.token_type_embeddings.weight"


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import multimodal_propaganda_meme_classification_amd as m
    return m


def _eq(a, b):
    """bit equality (floats compared on their int32 view: NaNs and the sign of zero count)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.detach().contiguous().reshape(-1), b.detach().contiguous().reshape(-1)
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    elif a.dtype in (torch.float16, torch.bfloat16):
        a, b = a.view(torch.int16), b.view(torch.int16)
    return torch.equal(a, b)


def _config(pkg, name):
    """name -> (ModelConfig dict, the config's own path)"""
    if name == "reference-dropout-bf16":
        d, features, _ = _cases(pkg)["tiny-cls-bf16-packed"]
        d = pkg.ModelConfig.from_dict(d).with_reference_dropout().to_dict()
        assert d["text"]["hidden_dropout"] > 0 and d["head_dropout"] > 0
    else:
        d, features, _ = _cases(pkg)[name]
    assert 64 <= d["text"]["vocab_size"] <= 600
    return d, ("sequence" if features == "sequence" else "encode" if features else "fused")


def _dropout(model):
    c = model.config
    return c.text.hidden_dropout > 0 or c.text.attention_dropout > 0 or c.head_dropout > 0


def _batch(cfg, B, S, seed, full=False):
    """[ids, image, mask, labels, w_t, w_i] on the device.  full: every row has all S tokens; otherwise ragged, row 0 full and (for
    B > 1) row 1 with ONE valid token.  Padded positions hold the pad id."""
    g = torch.Generator().manual_seed(seed)
    t, v = cfg.text, cfg.image
    ids = torch.randint(5, t.vocab_size, (B, S), generator=g)
    lens = torch.randint(2, S + 1, (B,), generator=g)
    lens[0] = S
    if B > 1:
        lens[1] = 1
    if full:
        lens[:] = S
    mask = (torch.arange(S)[None] < lens[:, None]).long()
    ids[:, 0] = 2
    ids = torch.where(mask.bool(), ids, torch.full_like(ids, t.pad_token_id))
    image = torch.randn((B, v.channels, v.image_size, v.image_size), generator=g)
    labels = torch.randint(0, cfg.num_classes, (B,), generator=g)
    w_t, w_i = torch.randn((B, S, t.hidden), generator=g), torch.randn((B, v.n_tokens, v.hidden), generator=g)
    return [x.cuda() for x in (ids, image, mask, labels, w_t, w_i)]


def _poisoned(cfg, B, S, seed):
    """an inf pixel in sample 1, as tests/test_scaler_gpu.py injects one: an ordinary overflow step (NaNs, no fault)"""
    mb = _batch(cfg, B, S, seed, full=True)
    mb[1][1, 0, 3, 3] = float("inf")
    return mb


def _run(pkg, model, path, mb, weight=1.0):
    """One forward + backward through a public entry point; returns clones of what the call hands back."""
    ids, image, mask, labels, w_t, w_i = mb
    if path == "fused":
        loss, ncorrect, logits = model.forward_backward(ids, image, mask, labels)
        out = dict(loss=loss, ncorrect=ncorrect, logits=logits)
    elif path == "autograd":
        crit = pkg.CrossEntropyLoss()
        logits = model(ids, image, mask)
        loss = crit(logits, labels) * weight
        loss.backward()
        out = dict(loss=loss, ncorrect=crit.last_correct, logits=logits)
    elif path == "encode":                      # a PyTorch head on the pooled features
        f_t, f_i = model.encode(ids, image, mask)
        loss = ((f_t * w_t[:, 0]).sum() + (f_i * w_i[:, 0]).sum()) * (weight * FEATURE_GRAD)
        loss.backward()
        out = dict(loss=loss, text_features=f_t, image_features=f_i)
    else:
        assert path == "sequence"
        h_t, h_i = model.encode_sequence(ids, image, mask)
        loss = ((h_t * w_t).sum() + (h_i * w_i).sum()) * (weight * FEATURE_GRAD)
        loss.backward()
        out = dict(loss=loss, text_states=h_t, image_states=h_i)
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in out.items()}


def _rows(mbs, cfg):
    """the word-table rows a list of batches gives a gradient to: ids under the mask, the pad id aside"""
    hit = torch.zeros(cfg.text.vocab_size, dtype=torch.bool)
    for mb in mbs:
        hit[mb[0][mb[2].bool()].cpu()] = True
    hit[cfg.text.pad_token_id] = False
    return hit


def _table(model, name):
    return dict(model.named_parameters())[name].grad


def _zero_facts(model, probe_mbs, path, who):
    """What has to be exactly 0.0 after the probe, whatever ran before (a NaN fails these comparisons as well)."""
    cfg = model.config
    S = max(mb[0].shape[1] for mb in probe_mbs)
    hit = _rows(probe_mbs, cfg).cuda()
    gw = _table(model, WORD)
    assert int((~hit).sum()) > 0 and float(gw[~hit].abs().max()) == 0.0, (who, "word-table rows outside the probe (or the pad row) hold a gradient",
                                                                       ((gw.abs().sum(1) != 0) & ~hit).nonzero().flatten().tolist()[:16])
    if cfg.text.position_scheme != "roberta":
        gp = _table(model, POS)
        assert S < gp.shape[0]
        assert float(gp[S:].abs().max()) == 0.0, (who, f"position-table rows >= {S} hold a gradient",
                                                  (gp[S:].abs().sum(1) != 0).nonzero().flatten().add(S).tolist())
    if cfg.text.type_vocab > 1:
        assert float(_table(model, TYPE)[1:].abs().max()) == 0.0, (who, "token-type rows >= 1 hold a gradient")
    if path in ("encode", "sequence"):
        for n, p in model.named_parameters():
            if n.startswith(HEAD):
                assert float(p.grad.abs().max()) == 0.0, (who, n, "the built-in head received a gradient on a features path")


def _live_everywhere(model, path, who):
    for n, p in model.named_parameters():
        assert bool(torch.isfinite(p.grad).all()), (who, n, "non-finite gradient after the probe")
        if ".key.bias" in n or (path in ("encode", "sequence") and n.startswith(HEAD)):
            continue
        assert float(p.grad.abs().sum()) > 0.0, (who, n, "all-zero gradient after the probe")


def _adam_state(model, opt):
    return dict(flat_params=model.flat_params, flat_shadow=model.flat_shadow, adam_m=opt._flat["M"], adam_v=opt._flat["V"])


def _twins(pkg, name, history, probe_shapes, path=None, accumulate=False, tag=""):
    """The twin protocol.  history(used model, its own path) runs on the used twin and returns the batches whose backward it ran;
    the probe is one batch per shape in probe_shapes -- one overwriting step, or with accumulate one window -- on `path` (default:
    the config's own)."""
    d, own = _config(pkg, name)
    path = path or own
    if accumulate and path == "fused":
        path = "autograd"               # forward_backward refuses a model that accumulates
    fresh, used = _model(pkg, d), _model(pkg, d)
    cfg = used.config
    assert _eq(fresh.flat_params, used.flat_params)
    p0 = used.flat_params.clone()
    hist_mbs = history(used, own)
    torch.cuda.synchronize()
    assert _eq(used.flat_params, p0) and not used.weights_changed(), "a history takes no optimizer step"
    hist_last = used.flat_grads.clone()
    probe_mbs = [_batch(cfg, B, S, seed=900 + k) for k, (B, S) in enumerate(probe_shapes)]
    extra = int((_rows(hist_mbs, cfg) & ~_rows(probe_mbs, cfg)).sum())
    parity_log(f"history independence {tag} {name}: word rows touched by the history and not by the probe: {extra}")
    assert extra >= 5, extra
    outs, opts = {}, {}
    for who, m in (("fresh", fresh), ("used", used)):
        opts[who] = pkg.Adam(m.parameters(), lr=LR)         # created after the history
        m.set_grad_accumulation(accumulate)
        if accumulate:
            opts[who].zero_grad()
        if _dropout(m):
            m.manual_seed(SEED)
        outs[who] = [_run(pkg, m, path, mb, weight=1.0 / len(probe_mbs)) for mb in probe_mbs]
    assert not _eq(hist_last, used.flat_grads), "the history left the probe's own gradient behind: nothing is tested"
    assert int(used._get_engine().word_row_live.sum()) > int(fresh._get_engine().word_row_live.sum())
    # facts that do not rest on the twin, then the twin comparison; a failure reports both
    problems = []
    for who, m in (("used", used), ("fresh", fresh)):
        try:
            _zero_facts(m, probe_mbs, path, who)
        except AssertionError as e:
            problems.append(("exact zero", str(e).splitlines()[0][:400]))
    _live_everywhere(fresh, path, "fresh")
    for k, (a, b) in enumerate(zip(outs["fresh"], outs["used"])):
        assert a.keys() == b.keys()
        problems += [("twin", f"probe batch {k}: {key} depends on the history") for key in a if not _eq(a[key], b[key])]
    bad = _report(used, used.flat_grads, fresh.flat_grads)
    if bad:
        problems.append(("twin", "gradients that depend on the history (name, differing elements, max |diff|)", bad))
    elif not _eq(used.flat_grads, fresh.flat_grads):
        problems.append(("twin", "the alignment padding of the flat gradient buffer depends on the history"))
    for (n, p), (n2, q) in zip(fresh.named_parameters(), used.named_parameters()):
        assert n == n2 and p.grad is not None and q.grad is not None
        if not _eq(p.grad, q.grad):
            problems.append(("twin", f"{n}.grad depends on the history"))
    assert not problems, (tag, name, problems)
    # one optimizer step: more word rows are marked live on the used model, where the step has to be the identity
    for who, m in (("fresh", fresh), ("used", used)):
        opts[who].step()
    torch.cuda.synchronize()
    a, b = _adam_state(fresh, opts["fresh"]), _adam_state(used, opts["used"])
    for key in a:
        assert _eq(a[key], b[key]), (tag, name, f"{key} after Adam.step() depends on the history")
    assert bool(torch.isfinite(used.flat_params).all()) and not _eq(used.flat_params, p0), "the step updated nothing"
    return fresh, used


# ---------------------------------------------------------------------------------------------------------------------------
# H1, H2, H5: every config
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CONFIGS)
def test_h1_longer_and_larger_batches_before(pkg, name):
    """(6, 16) then (4, 16), every row full length: every packed buffer, row count and position row is at its maximum before the
    probe (2, 9) shrinks them.  With the position rows [S, 16) left uncleared this fails on every absolute-position config, at the
    exact-zero assertion and at the twin comparison."""
    def history(m, own):
        mbs = [_batch(m.config, 6, 16, seed=11, full=True), _batch(m.config, 4, 16, seed=12, full=True)]
        for mb in mbs:
            _run(pkg, m, own, mb)
        return mbs
    _twins(pkg, name, history, [(2, 9)], tag="H1")


@pytest.mark.parametrize("name", CONFIGS)
def test_h2_same_shape_denser_mask_other_ids(pkg, name):
    """The probe's own plan object, reused with fewer live rows: the history is a (3, 12) batch of full rows and other ids, the probe
    a ragged (3, 12) batch whose row 1 has one valid token."""
    def history(m, own):
        mbs = [_batch(m.config, 3, 12, seed=21, full=True)]
        _run(pkg, m, own, mbs[0])
        return mbs
    fresh, used = _twins(pkg, name, history, [(3, 12)], tag="H2")
    assert len(used._get_engine().plans) == 1, "the history and the probe share one plan"


@pytest.mark.parametrize("name", CONFIGS)
def test_h5_poisoned_step_before(pkg, name):
    """An overflow step first: one forward_backward of shape (6, 16) whose image holds an inf pixel (on the features configs also
    one such step on their own path).  Any kernel that reads a row it should not -- a packed row past the live count, a beta = 0
    epilogue that still loads C, a stale split-K slab -- turns the probe's bits to NaN."""
    def history(m, own):
        mbs = [_poisoned(m.config, 6, 16, seed=51)]
        _run(pkg, m, "fused", mbs[0])
        if own != "fused":
            mbs.append(_poisoned(m.config, 6, 16, seed=52))
            _run(pkg, m, own, mbs[-1])
        bad = int((~torch.isfinite(m.flat_grads)).sum())
        parity_log(f"history independence H5 {name}: non-finite elements of flat_grads after the poisoned step: {bad} of {m.flat_grads.numel()}")
        assert bad > 0, "the poisoned history left no non-finite gradient"
        return mbs
    _twins(pkg, name, history, [(2, 9)], tag="H5")


# ---------------------------------------------------------------------------------------------------------------------------
# H3: entry-point switch under one (B, S)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["autograd", "encode", "sequence"])
@pytest.mark.parametrize("name", ["tiny-cls-bf16-packed", "text3-image2-dense", "features-pooled-fp16", "features-sequence-bf16"])
def test_h3_entry_point_switch_same_shape(pkg, name, path):
    """forward_backward, autograd model(...) + CrossEntropyLoss().backward(), encode(...) with a PyTorch head and encode_sequence(...)
    in a row under (3, 12), then the probe on one of the three autograd paths: four plans over the same flat gradient buffer (the head's
    slots are written by two of them and have to be zero after the other two)."""
    def history(m, own):
        mbs = [_batch(m.config, 3, 12, seed=31 + k, full=(k % 2 == 0)) for k in range(4)]
        for mb, p in zip(mbs, ("fused", "autograd", "encode", "sequence")):
            _run(pkg, m, p, mb)
        return mbs
    _twins(pkg, name, history, [(3, 12)], path=path, tag=f"H3->{path}")


# ---------------------------------------------------------------------------------------------------------------------------
# H4: mode switch
# ---------------------------------------------------------------------------------------------------------------------------
def _eval_calls(model, seed, shapes=((6, 16), (3, 12), (2, 9))):
    """forward-only use between training steps: eval() + no_grad forwards (the probe's shapes among them) and a get_features dump"""
    model.eval()
    with torch.no_grad():
        for k, (B, S) in enumerate(shapes):
            ids, image, mask = _batch(model.config, B, S, seed=seed + k, full=(k == 0))[:3]
            model(ids, image, mask)
    model.train()
    ids, image, mask = _batch(model.config, 4, 16, seed=seed + 7)[:3]
    feats = model.get_features(ids, image, mask)
    assert model.training and bool(torch.isfinite(feats["text"]).all())


@pytest.mark.parametrize("name", ["tiny-cls-bf16-packed", "reference-dropout-bf16"])
def test_h4_mode_switch(pkg, name):
    """eval() + no_grad forwards of other shapes and of the probe's, get_features(...), an eval() forward WITH grad and its backward,
    then back to train().  With dropout the train and eval plans are different objects; without, they are the same one."""
    def history(m, own):
        _eval_calls(m, seed=41)
        m.eval()
        mbs = [_batch(m.config, 6, 16, seed=49, full=True)]
        _run(pkg, m, "autograd", mbs[0])
        m.train()
        return mbs
    fresh, used = _twins(pkg, name, history, [(2, 9)], tag="H4")
    keys = list(used._get_engine().plans)
    assert (len({k[2] for k in keys}) == 2) == (name == "reference-dropout-bf16"), keys       # k[2]: the plan carries dropout


# ---------------------------------------------------------------------------------------------------------------------------
# H6, H7: accumulation windows
# ---------------------------------------------------------------------------------------------------------------------------
ACCUM_CONFIGS = ["tiny-cls-bf16-packed", "tiny-last-fp16-packed", "roberta-text"]


def _window(pkg, m, opt, own, shapes, seed):
    path = "autograd" if own == "fused" else own
    mbs = [_batch(m.config, B, S, seed=seed + k, full=True) for k, (B, S) in enumerate(shapes)]
    opt.zero_grad()
    for mb in mbs:
        _run(pkg, m, path, mb, weight=1.0 / len(mbs))
    return mbs


@pytest.mark.parametrize("order", ["long-first", "short-first"])
@pytest.mark.parametrize("name", ACCUM_CONFIGS)
def test_h6_accumulation_window_after_a_larger_window(pkg, name, order):
    """set_grad_accumulation(True): one complete window of (6, 16), (4, 16) and opt.zero_grad(), then the probe window (3, 12), (2, 9)
    -- and both windows in reverse order, where the adding backward is longer than the overwriting one."""
    flip = (lambda s: s) if order == "long-first" else (lambda s: s[::-1])

    def history(m, own):
        m.set_grad_accumulation(True)
        opt = pkg.Adam(m.parameters(), lr=LR)
        mbs = _window(pkg, m, opt, own, flip([(6, 16), (4, 16)]), seed=61)
        opt.zero_grad()
        return mbs
    _twins(pkg, name, history, flip([(3, 12), (2, 9)]), accumulate=True, tag=f"H6 {order}")


@pytest.mark.parametrize("name", ACCUM_CONFIGS)
def test_h7_accumulation_switched_on_then_off(pkg, name):
    """Accumulation on for one window, then off (no zero_grad in between: the window's rows are still there), then the probe with
    the switch off."""
    def history(m, own):
        m.set_grad_accumulation(True)
        mbs = _window(pkg, m, pkg.Adam(m.parameters(), lr=LR), own, [(4, 16), (6, 16)], seed=71)
        m.set_grad_accumulation(False)
        return mbs
    _twins(pkg, name, history, [(2, 9)], tag="H7")


# ---------------------------------------------------------------------------------------------------------------------------
# H8: GraphedStep (eager launches) with other work in between, and a third model beside it
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny-cls-bf16-packed", "tiny-last-fp16-packed"])
def test_h8_graphed_step_with_other_work_between_steps(pkg, name):
    """GraphedStep(model, opt, 3, 12, use_graph=False) on both twins, three steps on three batches.  Before every step the used twin
    also runs the forward-only calls of H4 (the step's own shape among them: without dropout that is the step's plan object), and a
    THIRD model runs an eager forward_backward of shape (6, 16): nothing is shared across model objects.  Parameters, shadow,
    moments, gradients, loss and correct count are compared after each step."""
    d, _ = _config(pkg, name)
    fresh, used, third = _model(pkg, d), _model(pkg, d), _model(pkg, d, seed=9)
    opts = [pkg.Adam(m.parameters(), lr=LR, model=m) for m in (fresh, used)]
    steps = [pkg.GraphedStep(m, o, 3, 12, use_graph=False) for m, o in zip((fresh, used), opts)]
    p0 = fresh.flat_params.clone()
    try:
        for k in range(3):
            _eval_calls(used, seed=81 + 10 * k)
            _run(pkg, third, "fused", _batch(third.config, 6, 16, seed=89 + k, full=True))
            ids, image, mask, labels = _batch(fresh.config, 3, 12, seed=800 + k)[:4]
            got = []
            for gs in steps:
                gs.load_batch(ids, image, mask, labels)
                loss, ncorrect = gs.step()
                torch.cuda.synchronize()
                got.append(dict(loss=loss.clone(), ncorrect=ncorrect.clone(), logits=gs.plan.buf["logits"].clone(),
                                flat_grads=gs.model.flat_grads.clone(), **_adam_state(gs.model, gs.opt)))
            for key in got[0]:
                assert _eq(got[0][key], got[1][key]), (name, f"step {k}: {key} depends on what ran between the steps")
            assert bool(torch.isfinite(got[1]["loss"]).all()) and bool(torch.isfinite(used.flat_params).all())
        assert not _eq(used.flat_params, p0)
    finally:
        for gs in steps:
            gs.close()


# ---------------------------------------------------------------------------------------------------------------------------
# H9: Kevin's three-tower model
# ---------------------------------------------------------------------------------------------------------------------------
def test_h9_kevins_model_small_last_batch_of_an_epoch(pkg):
    """KevinMultimodalClassifier("concatenation", image="resnet18") in train() with dropout 0: the history is (6, 16) then (2, 16)
    -- the small last batch of an epoch -- and the probe (4, 16).  BatchNorm normalises with batch statistics in train(), so the
    gradients carry no history (the running statistics do, and are not compared).  Every parameter's .grad of the three towers and
    the heads, bit for bit."""
    tc = pkg.TextConfig(vocab_size=600, hidden=128, layers=2, heads=2, intermediate=256, max_position=64)
    cc = pkg.TextConfig(vocab_size=500, hidden=128, layers=1, heads=2, intermediate=256, max_position=64)

    def make():
        m = pkg.KevinMultimodalClassifier("concatenation", text=tc, image="resnet18", caption=cc, proj=128, compute_dtype="bf16", seed=1,
                                          resnet_layers=(1, 1, 1, 1))
        m.text_dropout.p = m.caption_text_dropout.p = 0.0
        m.image_fine_tune[2].p = 0.0
        return m

    fresh, used = make(), make()
    fresh.cuda().train(), used.cuda().train()
    for (n, p), (n2, q) in zip(fresh.named_parameters(), used.named_parameters()):
        assert n == n2 and _eq(p, q), n
    crit = pkg.SigmoidFocalLoss()

    def mb(B, S, seed):
        g = torch.Generator().manual_seed(seed)
        text, cap = torch.randint(5, 600, (B, S), generator=g), torch.randint(5, 500, (B, S), generator=g)
        lens = torch.randint(1, S + 1, (B,), generator=g)
        mask = (torch.arange(S)[None] < lens[:, None]).long()
        image = torch.randn((B, 3, 64, 64), generator=g)
        labels = (torch.rand(B, generator=g) < 0.4).float()
        return [x.cuda() for x in (text * mask, image, mask, cap * mask, mask)], labels.cuda()

    def step(model, opt, batch):
        x, y = batch
        opt.zero_grad()
        logits = model(*x)
        loss = crit(logits, y, alpha=0.25, gamma=2.0, reduction="mean")
        loss.backward()
        torch.cuda.synchronize()
        return dict(logits=logits.detach().clone(), loss=loss.detach().clone())

    def grads(model):
        return {n: p.grad.detach().clone() for n, p in model.named_parameters()}

    o_fresh, o_used = (pkg.Adam(m.get_params(1e-4), lr=1e-4) for m in (fresh, used))
    for k, (B, S) in enumerate(((6, 16), (2, 16))):
        step(used, o_used, mb(B, S, seed=91 + k))
    last = grads(used)
    probe = mb(4, 16, seed=95)
    out_f, out_u = step(fresh, o_fresh, probe), step(used, o_used, probe)
    g_f, g_u = grads(fresh), grads(used)
    assert any(not _eq(last[n], g_u[n]) for n in g_u)
    assert all(bool(torch.isfinite(v).all()) for v in g_f.values()) and sum(float(v.abs().sum()) > 0 for v in g_f.values()) > 40
    for key in out_f:
        assert _eq(out_f[key], out_u[key]), key
    bad = [(n, int((g_f[n] != g_u[n]).sum()), float((g_f[n] - g_u[n]).abs().max())) for n in g_f if not _eq(g_f[n], g_u[n])]
    print("Kevin's model, gradients that depend on the history:", bad)
    assert not bad, bad
