"""The class-weighted / label-smoothed / ignore-index cross-entropy (mh_ce_opts_fwd_bwd) and the binary cross-entropy with a
positive-class weight (mh_bce_fwd_bwd) on the MI355X, from the kernels up to the fused step.

Reference: ``F.cross_entropy`` / ``F.binary_cross_entropy_with_logits`` in float64 on the CPU, through autograd, on the f32 values
the kernels read.  The bars are derived per element from the kernel's f32 evaluation (EPS32 = 2^-24, TRANS = 8 EPS32 for expf / logf /
log1pf), restating ``_ce_ref`` of tests/test_head_optim_paths_gpu.py and extending it:

  * lse_i:                      4 EPS32 (|max_i| + |lse_i - max_i|) + (C + 4) EPS32                           (as there)
  * n_i = lse_i - z_{i,c}:      4 EPS32 |z_{i,c}| + the lse bar                                               (as there)
  * a weight product w n:       w x (the bar of n) + EPS32 |w n|                                              (one rounding per factor)
  * the smoothing sum s_i = sum_c w_c (lse_i - z_{i,c}): the sum of its terms' bars + (C + 2) EPS32 sum_c |w_c (lse_i - z_{i,c})|
  * l_i = (1 - eps) w_y n_y + (eps / C) s_i: each product's bar times its coefficient + 4 EPS32 (|first| + |second|)
    (1 - eps and eps / C are rounded once each, the two products and the sum once each)
  * sum_i l_i:                  the sum of the rows' bars + (B + 2) EPS32 sum_i |l_i|
  * mean: the division by W = sum_i k_i w_{y_i}: (B + 2) EPS32 relative (W's own f32 sum) + 2 EPS32 (the division, the product)
  * p_{i,c} = exp(z - lse):     p (2 EPS32 (|z| + |lse|) + the lse bar + TRANS)                               (as there)
  * dlogits = [ (1 - eps) w_y (p - 1{c = y}) + (eps / C) (S_w p - w_c) ] inv,  S_w = sum_c w_c:
      first term   (1 - eps) w_y (p bar + EPS32 |p - 1|) + 3 EPS32 |term|
      second term  (eps / C) (S_w p bar + (C + 2) EPS32 S_w p + 2 EPS32 (S_w p + w_c)) + 3 EPS32 |term|
      times |inv|, plus 2 EPS32 (|first| + |second|) |inv|, plus |d| x (the relative bar of the division under "mean")
  * reduction "none" through the module: the per-row upstream gradient u_i is one more f32 product: bar |u_i| + EPS32 |d u_i|.
Every bar comes from the float64 reference and the number formats; none was fitted to what the kernels return.  The worst
error / bar ratio of every case goes through conftest.parity_log (profiles/r24_loss_options.txt); a ratio above 1 fails.

Bit-exact (no tolerance): the kernel without options == mh_ce_fwd_bwd; uniform weights of 2 == no weights (the power of two
cancels in every product and in the division); ignored rows are +0.0 and nothing is written past B x C; the fused step's loss job
== the stand-alone kernel on the plan's logits; the fused step under uniform weights of 2 == the plain fused step in every
parameter gradient; a captured step == the same step launched eagerly, with new weight values and a new label_smoothing in between;
an accumulation window under the weighted loss == the f32 sum of its micro-batches' gradients.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import parity_log

pytestmark = pytest.mark.gpu

F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
EPS32 = 2.0 ** -24
TRANS = 8 * EPS32
SENT32 = -7777.0
NEVER = -1_000_000          # torch's ignore_index when no label is ignored (no label has this value)


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.set_num_threads(16)
    import multimodal_propaganda_meme_classification_amd as m
    from multimodal_propaganda_meme_classification_amd import ops as _ops
    m.ops = _ops
    return m


def _f32(t64):
    return t64.to(F32).to(F64)


def _dev32(t64):
    return t64.to(F32).cuda().contiguous()


def _rand(shape, g, scale=1.0, shift=0.0):
    return _f32(torch.randn(shape, generator=g, dtype=F64) * scale + shift)


def _bits(t):
    return t.detach().cpu().contiguous().view(I32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _check(what, got, ref, bar):
    """|got - ref| <= bar elementwise.  Returns the worst error as a fraction of the bar."""
    got = got.detach().cpu().to(F64).reshape(ref.shape)
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite values"
    bar = torch.as_tensor(bar, dtype=F64).expand_as(ref) + 1e-37
    frac = (got - ref).abs() / bar
    worst = float(frac.max()) if frac.numel() else 0.0
    print(f"  {what}: worst error / bar {worst:.3e}")
    if worst > 1.0:
        i = int(frac.argmax())
        raise AssertionError(f"{what}: {int((frac > 1).sum())}/{frac.numel()} off; worst {worst:.3g} x bar (ref "
                             f"{float(ref.flatten()[i]):.6g}, got {float(got.flatten()[i]):.6g}, bar {float(bar.flatten()[i]):.3g})")
    return worst


def _log(tag, errs):
    parity_log(f"[lossopts {tag}] " + " ".join(f"{k} {x:.3e}" if isinstance(x, float) else f"{k} {x}" for k, x in errs.items()))


def _ignored_rows(B):
    """Rows 0 and B-1 plus every third row (B >= 3); B = 1 ignores nothing here (its all-ignored case is a test of its own)."""
    if B < 3:
        return []
    return sorted({0, B - 1} | set(range(0, B, 3)))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. mh_ce_opts_fwd_bwd against float64 torch
# ---------------------------------------------------------------------------------------------------------------------------------

CE_CASES = [(b, c) for b in (1, 63, 64, 65, 1024) for c in (1, 2, 5, 1000)]
CE_IDS = [f"B{b}_C{c}" for b, c in CE_CASES]

# name, weights, ignore, eps, reduction, logit offset, (grad_scale, device scale)
OPTION_SETS = [
    ("weights", True, False, 0.0, "mean", 0.0, (1.0, None)),
    ("weights_off+1e4_gs", True, False, 0.0, "mean", 1e4, (0.75, 96.0)),
    ("ignore", False, True, 0.0, "mean", 0.0, (1.0, None)),
    ("ignore_off-1e4_gs", False, True, 0.0, "mean", -1e4, (0.75, 96.0)),
    ("smooth0.1", False, False, 0.1, "mean", 0.0, (1.0, None)),
    ("smooth0.1_off+1e4", False, False, 0.1, "mean", 1e4, (1.0, None)),
    ("smooth1_gs", False, False, 1.0, "mean", 0.0, (0.75, 96.0)),
    ("all", True, True, 0.1, "mean", 0.0, (1.0, None)),
    ("all_off+1e4_gs", True, True, 0.1, "mean", 1e4, (0.75, 96.0)),
    ("all_off-1e4", True, True, 0.1, "mean", -1e4, (1.0, None)),
    ("all_smooth1", True, True, 1.0, "mean", 0.0, (1.0, None)),
    ("sum", True, True, 0.1, "sum", 0.0, (0.75, 96.0)),
    ("sum_off-1e4", True, True, 0.1, "sum", -1e4, (1.0, None)),
    ("none", True, True, 0.1, "none", 0.0, (0.75, 96.0)),
    ("none_off+1e4", True, True, 0.1, "none", 1e4, (1.0, None)),
]


def _ce_opts_ref(z, y, w, ign, eps, reduction, scale):
    """float64 reference of the f32 logits z: (loss, loss bar, dlogits, dlogits bar, n_correct).  ``w`` float64 [C] or None,
    ``ign`` the ignored label or None, ``eps`` the f32 value of label_smoothing as float64, ``scale`` the f32 gradient scale.
    The loss and its gradient are torch's (autograd); the closed form below only carries the bars, and is asserted to agree."""
    B, Cn = z.shape
    zr = z.clone().requires_grad_(True)
    out = F.cross_entropy(zr, y, weight=w, ignore_index=NEVER if ign is None else ign, label_smoothing=eps, reduction=reduction)
    (out.sum() * scale).backward()        # "none": each row's own derivative (upstream gradient 1 per row)
    loss_t, d_t = out.detach(), zr.grad
    keep = torch.ones(B, dtype=torch.bool) if ign is None else (y != ign)
    yc = torch.where((y < 0) | (y >= Cn), torch.zeros_like(y), y)
    wv = torch.ones(Cn, dtype=F64) if w is None else w
    wy = wv[yc]
    rows = torch.arange(B)
    mx = z.max(1).values
    lse = mx + torch.log(torch.exp(z - mx[:, None]).sum(1))
    lse_bar = 4 * EPS32 * (mx.abs() + (lse - mx).abs()) + (Cn + 4) * EPS32
    n = lse[:, None] - z                                              # [B][C]
    n_bar = 4 * EPS32 * z.abs() + lse_bar[:, None]
    t1 = wy * n[rows, yc]
    t1_bar = wy * n_bar[rows, yc] + EPS32 * t1.abs()
    terms = wv[None] * n
    s1 = terms.sum(1)
    s1_bar = (wv[None] * n_bar + EPS32 * terms.abs()).sum(1) + (Cn + 2) * EPS32 * terms.abs().sum(1)
    a, e = 1.0 - eps, eps / Cn
    if eps == 0.0:
        li, li_bar = t1, t1_bar
    else:
        li = a * t1 + e * s1
        li_bar = a * t1_bar + e * s1_bar + 4 * EPS32 * ((a * t1).abs() + (e * s1).abs())
    li, li_bar = li * keep, li_bar * keep
    W = float((wy * keep).sum())
    sum_bar = float(li_bar.sum() + (B + 2) * EPS32 * li.abs().sum())
    div_rel = (B + 2) * EPS32 + 2 * EPS32
    if reduction == "mean":
        loss, loss_bar = li.sum() / W, sum_bar / W + div_rel * abs(float(li.sum() / W))
        inv, inv_rel = scale / W, div_rel
    elif reduction == "sum":
        loss, loss_bar, inv, inv_rel = li.sum(), sum_bar, scale, 0.0
    else:
        loss, loss_bar, inv, inv_rel = li, li_bar, scale, 0.0
    # (float64 itself keeps 2^-52 of the logits' magnitude per row, far below every bar)
    slack = 1e-11 * (1 + float(z.abs().max())) * (1 + float(wv.max())) * (B if reduction == "sum" else 1)
    assert bool(((loss - loss_t).abs() <= 1e-9 * loss_t.abs() + slack).all()), "the closed form behind the bars is not torch's loss"
    p = torch.exp(z - lse[:, None])
    p_bar = p * (2 * EPS32 * (z.abs() + lse.abs()[:, None]) + lse_bar[:, None] + TRANS)
    oh = torch.zeros_like(z)
    oh[rows, yc] = 1.0
    Sw = float(wv.sum())
    first = a * wy[:, None] * (p - oh)
    first_bar = a * wy[:, None] * (p_bar + EPS32 * (p - oh).abs()) + 3 * EPS32 * first.abs()
    second = e * (Sw * p - wv[None])
    second_bar = e * (Sw * p_bar + (Cn + 2) * EPS32 * Sw * p + 2 * EPS32 * (Sw * p + wv[None])) + 3 * EPS32 * second.abs()
    d = (first + second) * inv * keep[:, None]
    assert bool(((d - d_t).abs() <= 1e-9 * (a * wy[:, None] * (p + oh) + e * (Sw * p + wv[None]) + 1e-6) * abs(inv)).all()), \
        "the closed form behind the bars is not torch's gradient"
    d_bar = (abs(inv) * (first_bar + second_bar + 2 * EPS32 * (first.abs() + second.abs())) + inv_rel * d.abs()) * keep[:, None]
    ncorrect = int(((z.argmax(1) == yc) & keep).sum())
    return loss_t, loss_bar, d_t, d_bar, ncorrect


def _weights(Cn, g, zero=True):
    """f32-representable positive class weights, one of them exactly 0 (C >= 2: with one class a zero weight is the 0 / 0 of the
    all-ignored case)."""
    w = _f32(torch.rand(Cn, generator=g, dtype=F64) * 2.5 + 0.25)
    if zero and Cn >= 2:
        w[Cn // 2] = 0.0
    return w


def _ce_inputs(B, Cn, g, offset, ignore):
    """Logits, labels and the ignored label.  The first kept row is labelled class 0, whose weight is never the zero one: the weight
    sum of the kept rows (the denominator of "mean") is positive by construction."""
    z = _rand((B, Cn), g, 3.0, offset)
    y = torch.randint(0, Cn, (B,), generator=g)
    ign = None
    rows = _ignored_rows(B) if ignore else []
    if ignore:
        ign = -100
        y[rows] = ign
    y[min(set(range(B)) - set(rows))] = 0
    return z, y, ign


def _run_ce_opts(pkg, z, y, w, ign, eps, reduction, gs=1.0, gsd=None, pad=0):
    B, Cn = z.shape
    loss = torch.full((B if reduction == "none" else 1,), SENT32, dtype=F32, device="cuda")
    dl = torch.full((B * Cn + pad,), SENT32, dtype=F32, device="cuda")
    nc = torch.full((1,), -5, dtype=I32, device="cuda")
    pkg.ops.ce_opts_fwd_bwd(_dev32(z), y.cuda(), loss, dl, nc, class_weight=None if w is None else _dev32(w), ignore_index=ign,
                            label_smoothing=eps, reduction=reduction, grad_scale=gs,
                            grad_scale_dev=None if gsd is None else torch.tensor([gsd], dtype=F32, device="cuda"))
    torch.cuda.synchronize()
    return loss, dl, nc


@pytest.mark.parametrize("B,Cn", CE_CASES, ids=CE_IDS)
def test_ce_opts_against_float64(pkg, B, Cn):
    """Every option set at every wave / workgroup edge, loss and every dlogits element inside its derived bar."""
    g = torch.Generator().manual_seed(2400 + B + Cn)
    errs = {}
    for name, weighted, ignore, eps, reduction, offset, (gs, gsd) in OPTION_SETS:
        z, y, ign = _ce_inputs(B, Cn, g, offset, ignore)
        w = _weights(Cn, g) if weighted else None
        eps64 = float(np.float32(eps))
        scale = float(np.float32(gs) * (np.float32(gsd) if gsd is not None else np.float32(1)))
        loss, dl, nc = _run_ce_opts(pkg, z, y, w, ign, eps, reduction, gs, gsd)
        loss_r, lbar, d_r, dbar, nc_r = _ce_opts_ref(z, y, w, ign, eps64, reduction, scale)
        errs[f"loss_{name}"] = _check(f"ce_opts B{B} C{Cn} loss {name}", loss, loss_r.reshape(-1), lbar)
        errs[f"dlogits_{name}"] = _check(f"ce_opts B{B} C{Cn} dlogits {name}", dl.view(B, Cn), d_r, dbar)
        assert int(nc) == nc_r, f"n_correct {name}"
    if Cn == 1:     # the single weight exactly 0: the mean is 0 / 0, in torch too
        z, y, _ = _ce_inputs(B, Cn, g, 0.0, False)
        loss, _, nc = _run_ce_opts(pkg, z, y, torch.zeros(1, dtype=F64), None, 0.0, "mean")
        ref = F.cross_entropy(z, y, weight=torch.zeros(1, dtype=F64))
        assert bool(torch.isnan(ref)) and bool(torch.isnan(loss).all())
    _log(f"ce_opts B{B} C{Cn}", errs)


@pytest.mark.parametrize("B,Cn", CE_CASES, ids=CE_IDS)
def test_ce_module_none_with_upstream_gradient(pkg, B, Cn):
    """CrossEntropyLoss(reduction="none") through autograd: [B] losses, and a non-uniform per-row upstream gradient multiplied in."""
    g = torch.Generator().manual_seed(2500 + B + Cn)
    z, y, ign = _ce_inputs(B, Cn, g, 0.0, True)
    w = _weights(Cn, g)
    u = _rand((B,), g, 1.5)
    eps = 0.1
    crit = pkg.CrossEntropyLoss(weight=w, ignore_index=ign, label_smoothing=eps, reduction="none").cuda()
    zd = _dev32(z).requires_grad_(True)
    out = crit(zd, y.cuda())
    assert tuple(out.shape) == (B,)
    out.backward(_dev32(u))
    torch.cuda.synchronize()
    loss_r, lbar, d_r, dbar, nc_r = _ce_opts_ref(z, y, w, ign, float(np.float32(eps)), "none", 1.0)
    errs = {"loss": _check("module none loss", out, loss_r, lbar),
            "grad": _check("module none grad", zd.grad, d_r * u[:, None], dbar * u.abs()[:, None] + EPS32 * (d_r * u[:, None]).abs())}
    assert int(crit.last_correct) == nc_r
    _log(f"ce_module_none B{B} C{Cn}", errs)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. mh_ce_opts_fwd_bwd, exact
# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,Cn", CE_CASES, ids=CE_IDS)
def test_ce_opts_without_options_is_ce_bit_for_bit(pkg, B, Cn):
    """No weights, no smoothing, no ignored label, "mean": the bits of mh_ce_fwd_bwd in loss, dlogits and n_correct (also with an
    ignore index set that no label carries, and with out-of-range labels, which both read as class 0)."""
    g = torch.Generator().manual_seed(2600 + B + Cn)
    for k, (offset, gs, gsd) in enumerate(((0.0, 1.0, None), (1e4, 0.75, 96.0), (-1e4, 1.0, None))):
        z = _rand((B, Cn), g, 3.0, offset)
        y = torch.randint(0, Cn, (B,), generator=g)
        if k == 2:
            y[::4] = 7 * Cn             # out of range, not the ignore index: class 0 in both kernels
        gdev = None if gsd is None else torch.tensor([gsd], dtype=F32, device="cuda")
        loss0 = torch.empty(1, dtype=F32, device="cuda")
        dl0 = torch.empty((B, Cn), dtype=F32, device="cuda")
        nc0 = torch.empty(1, dtype=I32, device="cuda")
        pkg.ops.ce_fwd_bwd(_dev32(z), y.cuda(), loss0, dl0, nc0, grad_scale=gs, grad_scale_dev=gdev)
        for ign in (None, -100):
            loss, dl, nc = _run_ce_opts(pkg, z, y, None, ign, 0.0, "mean", gs, gsd)
            assert _same_bits(loss, loss0) and _same_bits(dl.view(B, Cn), dl0) and int(nc) == int(nc0), (offset, ign)


@pytest.mark.parametrize("B,Cn", CE_CASES, ids=CE_IDS)
def test_ce_opts_uniform_weights_of_two_cancel_bit_for_bit(pkg, B, Cn):
    """Uniform weights of 2.0 under "mean": every product doubles exactly and the weight sum halves it back."""
    g = torch.Generator().manual_seed(2700 + B + Cn)
    z, y, ign = _ce_inputs(B, Cn, g, 0.0, B >= 3)
    two = torch.full((Cn,), 2.0, dtype=F64)
    a = _run_ce_opts(pkg, z, y, None, ign, 0.0, "mean", 0.75, 96.0)
    b = _run_ce_opts(pkg, z, y, two, ign, 0.0, "mean", 0.75, 96.0)
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1]) and int(a[2]) == int(b[2])


@pytest.mark.parametrize("B,Cn", [(63, 5), (65, 2), (1024, 1000)], ids=["B63_C5", "B65_C2", "B1024_C1000"])
def test_ce_opts_ignored_rows_are_positive_zero_and_nothing_else_is_written(pkg, B, Cn):
    g = torch.Generator().manual_seed(2800 + B + Cn)
    z, y, ign = _ce_inputs(B, Cn, g, 0.0, True)
    PAD = 64
    for w, eps, reduction in ((None, 0.0, "mean"), (_weights(Cn, g), 0.1, "mean"), (_weights(Cn, g), 0.1, "none")):
        loss, dl, nc = _run_ce_opts(pkg, z, y, w, ign, eps, reduction, pad=PAD)
        rows = torch.tensor(_ignored_rows(B))
        assert bool((_bits(dl[:B * Cn].view(B, Cn))[rows] == 0).all()), "an ignored row is not +0.0"
        assert bool((dl[B * Cn:] == SENT32).all()), "written past B x C"
        kept = torch.ones(B, dtype=torch.bool)
        kept[rows] = False
        assert bool((dl[:B * Cn].view(B, Cn).cpu()[kept] != SENT32).all()), "a kept row was not written"
        if reduction == "none":
            assert bool((_bits(loss)[rows] == 0).all())


@pytest.mark.parametrize("B,Cn", [(1, 2), (1, 1), (65, 5)], ids=["B1_C2", "B1_C1", "B65_C5"])
def test_ce_opts_all_rows_ignored(pkg, B, Cn):
    """torch's result: the mean is 0 / 0 = NaN; every gradient is zero; nothing counts as correct.  "sum" gives 0."""
    g = torch.Generator().manual_seed(2900 + B + Cn)
    z = _rand((B, Cn), g, 3.0)
    y = torch.full((B,), -100, dtype=I64)
    assert bool(torch.isnan(F.cross_entropy(z, y, ignore_index=-100)))
    for w, eps in ((None, 0.0), (_weights(Cn, g, zero=False), 0.1)):
        loss, dl, nc = _run_ce_opts(pkg, z, y, w, -100, eps, "mean", pad=8)
        assert bool(torch.isnan(loss).all()) and bool((_bits(dl[:B * Cn]) == 0).all()) and int(nc) == 0
        assert bool((dl[B * Cn:] == SENT32).all())
        loss, dl, nc = _run_ce_opts(pkg, z, y, w, -100, eps, "sum")
        assert float(loss) == 0.0 and bool((_bits(dl) == 0).all()) and int(nc) == 0


def test_ce_opts_refusals(pkg):
    lib = pkg._lib.load()
    st = torch.cuda.current_stream().cuda_stream
    z, y = torch.zeros((4, 3), device="cuda"), torch.zeros(4, dtype=I64, device="cuda")
    loss, dl = torch.zeros(4, device="cuda"), torch.zeros((4, 3), device="cuda")
    args = lambda eps, red, B=4: (z.data_ptr(), y.data_ptr(), None, loss.data_ptr(), dl.data_ptr(), None, B, 3, 0, 0, eps, red, 1.0, None, st)
    assert lib.mh_ce_opts_fwd_bwd(*args(0.0, 0)) == 0
    for eps, red, B in ((-0.01, 0, 4), (1.01, 0, 4), (float("nan"), 0, 4), (0.0, 3, 4), (0.0, -1, 4), (0.0, 0, 0), (0.0, 0, 1025)):
        assert lib.mh_ce_opts_fwd_bwd(*args(eps, red, B)) == pkg._lib.MH_ESHAPE, (eps, red, B)
    assert lib.mh_bce_fwd_bwd(z.data_ptr(), 1, loss.data_ptr(), 1.0, loss.data_ptr(), dl.data_ptr(), None, 4, 2, 1.0, None, st) == pkg._lib.MH_ESHAPE
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        pkg.CrossEntropyLoss(weight=[1.0, 2.0]).cuda()(torch.zeros((2, 3), device="cuda"), torch.zeros(2, dtype=I64, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. mh_bce_fwd_bwd
# ---------------------------------------------------------------------------------------------------------------------------------

BCE_CASES = [(b, ld, pw) for b in (1, 65, 999) for ld in (1, 3) for pw in (1.0, 0.25, 3.0)]
EDGES = [0.0, 1e-3, -1e-3, 17.0, -17.0, 30.0, -30.0, 88.5, -88.5]


def _bce_inputs(B, g):
    x = _f32(torch.cat([torch.tensor(EDGES, dtype=F64), torch.rand(max(B - len(EDGES), 0), generator=g, dtype=F64) * 60 - 30]))
    x = x[torch.randperm(x.numel(), generator=g)] if B >= len(EDGES) else x
    # B < 9: one row per run over the edge values (see the loop in the test)
    t = _f32(torch.tensor([0.0, 1.0, 0.3], dtype=F64))[torch.randint(0, 3, (x.numel(),), generator=g)]
    return x, t


def _bce_ref(x, t, pw, reduction, scale):
    """float64 torch through autograd, and the bars of the kernel's f32 evaluation: e = exp(-|x|), L = log1p(e), softplus(+-x) =
    max(+-x, 0) + L, the two sigmoids 1 / (1 + e) and e / (1 + e): every one a few f32 operations on positive terms, so each
    carries a RELATIVE error: TRANS for expf and for log1pf, and the error of e moves L by at most e x TRANS <= 2 L x TRANS
    (log1p(e) >= e / 2 on [0, 1]), so L -- the larger part of the chain -- is within 3 TRANS; the sum with max(+-x, 0), the two
    coefficients' products and the final sum add 4 EPS32.  REL = 3 TRANS + 4 EPS32 per term of the loss and of the gradient, with the
    terms' absolute values summed, so cancellation between the two terms is paid for; the gradient's scale product and division add
    4 EPS32 of the result.  Below the smallest normal f32 (2^-126: exp(-88.5) = 3.7e-39 is under it) a value may be flushed to zero or
    lose bits: TINY = 2^-126 absolute per term.  The float64 REFERENCE's own gradient is sigmoid(x) - t style arithmetic through autograd,
    which cancels for large |x| (1 - 1 / (1 + 5e-12) keeps 2^-52 of 1, not of 5e-12): 4 x 2^-52 (1 + pw) absolute per element; its
    loss is (1 - t) x + (1 + (pw - 1) t) (max(-x, 0) + log(exp(-max) + exp(-x - max))), which at x = -30, t = 0 adds -30 + 30 + 9.4e-14
    and keeps 2^-52 of 30: 4 x 2^-52 (1 + |x|) (1 + pw) absolute per element (seen: 9.237e-14 from torch, 9.3576e-14 = exp(-30) here)."""
    B = x.numel()
    xr = x.clone().requires_grad_(True)
    out = F.binary_cross_entropy_with_logits(xr, t, pos_weight=torch.tensor([pw], dtype=F64), reduction=reduction)
    (out * scale).backward()
    den = B if reduction == "mean" else 1
    with torch.no_grad():
        sp, sn = F.softplus(x), F.softplus(-x)
        terms = (1 - t) * sp + pw * t * sn                      # both terms >= 0
        REL, TINY = 3 * TRANS + 4 * EPS32, 2.0 ** -126
        lbar = float((REL * terms + (1 + pw) * (TINY + 4 * 2.0 ** -52 * (1 + x.abs()))).sum() + (B + 2) * EPS32 * terms.sum()) / den
        gterms = (1 - t) * torch.sigmoid(x) + pw * t * torch.sigmoid(-x)
        gbar = (REL * gterms + (1 + pw) * (TINY + 4 * 2.0 ** -52)) * abs(scale) / den + 4 * EPS32 * xr.grad.abs()
    return out.detach(), lbar, xr.grad, gbar


@pytest.mark.parametrize("B,ld,pw", BCE_CASES, ids=[f"B{b}_ld{ld}_pw{pw:g}" for b, ld, pw in BCE_CASES])
def test_bce_against_float64(pkg, B, ld, pw):
    g = torch.Generator().manual_seed(3000 + B + ld + int(100 * pw))
    errs = {}
    runs = len(EDGES) if B < len(EDGES) else 1          # B = 1: one launch per edge value
    for r in range(runs):
        for reduction, (gs, gsd) in (("mean", (4.0, None)), ("sum", (0.75, 96.0))):
            x, t = _bce_inputs(B, g)
            if runs > 1:
                x, t = x[r:r + B], t[r:r + B]
            scale = float(np.float32(gs) * (np.float32(gsd) if gsd is not None else np.float32(1)))
            xd = torch.full((B, ld), SENT32, dtype=F32, device="cuda")
            xd[:, 0] = _dev32(x)
            loss = torch.empty(1, dtype=F32, device="cuda")
            dl = torch.full((B, ld), SENT32, dtype=F32, device="cuda")
            nc = torch.empty(1, dtype=I32, device="cuda")
            pkg.ops.bce_fwd_bwd(xd, _dev32(t), loss, dl, nc, pos_weight=pw, reduction=reduction, grad_scale=gs,
                                grad_scale_dev=None if gsd is None else torch.tensor([gsd], dtype=F32, device="cuda"), ld=ld)
            torch.cuda.synchronize()
            loss_r, lbar, d_r, gbar = _bce_ref(x, t, pw, reduction, scale)
            k = f"{reduction}" + (f"_x{float(x[0]):g}" if runs > 1 else "")
            errs[f"loss_{k}"] = max(errs.get(f"loss_{k}", 0.0), _check(f"bce loss {k}", loss, loss_r.reshape(1), lbar))
            errs[f"dlogits_{k}"] = max(errs.get(f"dlogits_{k}", 0.0), _check(f"bce dlogits {k}", dl[:, 0], d_r, gbar))
            assert int(nc) == int(((x > 0) == (t > 0.5)).sum())
            assert bool((dl[:, 1:] == SENT32).all()), "written between the strided logits"
    _log(f"bce B{B} ld{ld} pw{pw:g}", errs)


@pytest.mark.parametrize("B", [1, 65, 999])
def test_bce_pos_weight_one_against_focal(pkg, B):
    """pos_weight = 1 is the focal kernel's alpha = -1, gamma = 0 on hard targets.  The LOSS is the same bits: softplus(+-x) here and
    max(x, 0) - x t + log1p(exp(-|x|)) there round identically when t is 0 or 1 (one of the two terms is exactly 0).  The GRADIENT is
    held to the sum of the two kernels' derived bars, not to equal bits: this kernel forms sigmoid(-x) from exp(-|x|) where the focal
    kernel forms p - t from one sigmoid, which cancels for large |x|."""
    g = torch.Generator().manual_seed(3100 + B)
    x, _ = _bce_inputs(max(B, len(EDGES)), g)
    x = x[:B]
    t = (torch.rand(B, generator=g) < 0.4).to(F64)
    outs = []
    for fn, kw in ((pkg.ops.bce_fwd_bwd, dict(pos_weight=1.0)), (pkg.ops.focal_fwd_bwd, dict(alpha=-1.0, gamma=0.0))):
        loss = torch.empty(1, dtype=F32, device="cuda")
        dl = torch.empty(B, dtype=F32, device="cuda")
        nc = torch.empty(1, dtype=I32, device="cuda")
        fn(_dev32(x), _dev32(t), loss, dl, nc, grad_scale=4.0, **kw)
        torch.cuda.synchronize()
        outs.append((loss, dl, int(nc)))
    assert _same_bits(outs[0][0], outs[1][0]), "loss bits"
    assert outs[0][2] == outs[1][2]
    _, _, d_r, gbar = _bce_ref(x, t, 1.0, "mean", 4.0)
    focal_bar = (16 * EPS32 * d_r.abs() + 4 * EPS32 * 4.0 / B * (1 + F.binary_cross_entropy_with_logits(x, t, reduction="none")))
    worst = _check("bce vs focal dlogits", outs[0][1], outs[1][1].cpu().to(F64), gbar + focal_bar)
    _log(f"bce_vs_focal B{B}", {"loss": "bit-exact", "dlogits": worst})


def test_bce_module(pkg):
    """BCEWithLogitsLoss: criterion(output, labels) on [B, 1] logits, the focal call's keywords accepted, autograd gradient."""
    g = torch.Generator().manual_seed(3200)
    B = 37
    x, t = _rand((B, 1), g, 3.0), (torch.rand(B, generator=g) < 0.3).to(F64)
    crit = pkg.BCEWithLogitsLoss(pos_weight=2.5)
    xd = _dev32(x).requires_grad_(True)
    loss = crit(xd, t.to(F32).cuda(), alpha=0.25, gamma=2.0, reduction="mean")
    (loss * 3.0).backward()
    torch.cuda.synchronize()
    loss_r, lbar, d_r, gbar = _bce_ref(x.view(-1), t, 2.5, "mean", 3.0)
    _check("bce module loss", loss.reshape(1), loss_r.reshape(1), lbar)
    _check("bce module grad", xd.grad.view(-1), d_r, gbar + EPS32 * d_r.abs())
    assert tuple(xd.grad.shape) == (B, 1)
    assert int(crit.last_correct) == int(((x.view(-1) > 0) == (t > 0.5)).sum())
    with pytest.raises(ValueError):
        crit(xd, t.to(F32).cuda(), reduction="sum")


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the fused step
# ---------------------------------------------------------------------------------------------------------------------------------

LR = 2e-5
S = 12


def _tiny_dict(pool="cls"):
    from oracle import meme_oracle as O
    return O.tiny_config(pool).to_dict()


def _model(pkg, seed=7):
    cfg = pkg.ModelConfig.from_dict(_tiny_dict())
    m = pkg.MultimodalClassifier.from_config(cfg, seed=seed)
    with torch.no_grad():       # biases and LayerNorm parameters away from their 0 / 1 initial values
        gen = torch.Generator().manual_seed(seed + 1)
        for n, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=gen) * 0.05)
    m.mark_weights_changed()
    return m.to("cuda").train()


def _batch(cfg, B, S_, seed, ignore=False):
    g = torch.Generator().manual_seed(seed)
    t, v = cfg.text, cfg.image
    ids = torch.randint(5, t.vocab_size, (B, S_), generator=g)
    lens = torch.randint(2, S_ + 1, (B,), generator=g)
    lens[0] = S_
    mask = (torch.arange(S_)[None] < lens[:, None]).long()
    ids[:, 0] = 2
    ids = torch.where(mask.bool(), ids, torch.full_like(ids, t.pad_token_id))
    image = torch.randn((B, v.channels, v.image_size, v.image_size), generator=g)
    labels = torch.randint(0, cfg.num_classes, (B,), generator=g)
    if ignore:
        labels[_ignored_rows(B)] = -100
    return [x.cuda() for x in (ids, image, mask, labels)]


W_A, W_B = [0.7142857313156128, 1.6666666269302368], [2.25, 0.5]


@pytest.mark.parametrize("B", [5, 64])
@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_fused_step_loss_job_is_the_standalone_kernel(pkg, B, reduction):
    """forward_backward with options: the plan's loss and dlogits are the bits of mh_ce_opts_fwd_bwd on the plan's logits (everything
    downstream of dlogits is the unchanged backward)."""
    model = _model(pkg)
    opts = dict(weight=W_A, ignore_index=-100, label_smoothing=0.1, reduction=reduction)
    assert model.set_loss_options(**opts) is model
    ids, image, mask, labels = _batch(model.config, B, S, 40 + B, ignore=True)
    loss, nc, logits = model.forward_backward(ids, image, mask, labels)
    torch.cuda.synchronize()
    eng = model._get_engine()
    plan = eng.plan(B, S, True)
    assert plan.loss_opts == model.loss_options and [c.name for c in plan.loss.calls] == ["mh_ce_opts_fwd_bwd"]
    assert loss.data_ptr() == plan.buf["loss"].data_ptr()
    want_loss = torch.empty(1, device="cuda")
    want_dl = torch.empty_like(plan.buf["dlogits"])
    want_nc = torch.empty(1, dtype=I32, device="cuda")
    pkg.ops.ce_opts_fwd_bwd(plan.buf["logits"].clone(), labels, want_loss, want_dl, want_nc, class_weight=torch.tensor(W_A, device="cuda"),
                            ignore_index=-100, label_smoothing=0.1, reduction=reduction, grad_scale=1.0, grad_scale_dev=eng.loss_scale)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want_loss).all()) and float(want_dl.abs().sum()) > 0
    assert _same_bits(plan.buf["loss"], want_loss) and _same_bits(plan.buf["dlogits"], want_dl) and int(nc) == int(want_nc)
    assert bool((_bits(plan.buf["dlogits"])[_ignored_rows(B)] == 0).all())
    assert float(model.flat_grads.abs().sum()) > 0 and bool(torch.isfinite(model.flat_grads).all())


def test_fused_step_without_options_is_built_as_before(pkg):
    """No options (never set, or set back to the defaults): the plan's key has no loss entry and its loss job is mh_ce_fwd_bwd."""
    model = _model(pkg)
    ids, image, mask, labels = _batch(model.config, 5, S, 45)
    model.forward_backward(ids, image, mask, labels)
    eng = model._get_engine()
    keys = list(eng.plans)
    plan = eng.plan(5, S, True)
    assert [c.name for c in plan.loss.calls] == ["mh_ce_fwd_bwd"] and plan.loss_opts is None
    model.set_loss_options(label_smoothing=0.2)
    assert eng.plan(5, S, True) is not plan and len(eng.plans) == 2
    model.set_loss_options()
    assert model.loss_options is None and model._get_engine().plan(5, S, True) is plan and list(eng.plans)[:1] == keys
    with pytest.raises(ValueError):
        model.set_loss_options(reduction="none")
    with pytest.raises(ValueError):
        model.set_loss_options(weight=[1.0, 2.0, 3.0])


@pytest.mark.parametrize("B", [5, 64])
def test_fused_step_uniform_weights_of_two_change_no_gradient_bit(pkg, B):
    model = _model(pkg)
    ids, image, mask, labels = _batch(model.config, B, S, 50 + B)
    loss, _, _ = model.forward_backward(ids, image, mask, labels)
    torch.cuda.synchronize()
    want, want_loss = model.flat_grads.clone(), loss.clone()
    model.set_loss_options(weight=[2.0, 2.0])
    model.flat_grads.zero_()
    loss, _, _ = model.forward_backward(ids, image, mask, labels)
    torch.cuda.synchronize()
    assert float(want.abs().sum()) > 0
    assert _same_bits(loss, want_loss) and _same_bits(model.flat_grads, want)


def test_graphed_step_follows_weights_and_label_smoothing(pkg):
    """A captured step against the same step launched eagerly on a fresh model (GraphedStep(use_graph=False): the same schedule,
    no capture), bit for bit in loss, n_correct, gradients and parameters: two replays with different labels and new class-weight
    VALUES in between (copied into the buffer the captured launch reads: the graphs are kept), then a new label_smoothing (another
    plan: the step drops its capture), then the first options again."""
    B = 5
    runs = []
    for use_graph in (True, False):
        model = _model(pkg)
        model.set_loss_options(weight=W_A, ignore_index=-100, label_smoothing=0.1)
        opt = pkg.Adam(model.parameters(), lr=LR)
        step = pkg.GraphedStep(model, opt, B, S, use_graph=use_graph)
        out = []
        script = [(60, None), (61, dict(weight=W_B, ignore_index=-100, label_smoothing=0.1)),
                  (62, dict(weight=W_B, ignore_index=-100, label_smoothing=0.3)), (63, dict(weight=W_A, ignore_index=-100, label_smoothing=0.1))]
        graphs = []
        for seed, opts in script:
            if opts is not None:
                model.set_loss_options(**opts)
            step.load_batch(*_batch(model.config, B, S, seed, ignore=True))
            loss, nc = step.step()
            torch.cuda.synchronize()
            graphs.append(step.graphs)
            out.append((loss.clone(), nc.clone(), step.plan.buf["dlogits"].clone(), model.flat_grads.clone(), model.flat_params.clone()))
        if use_graph:
            assert graphs[0] is not None and graphs[1] is graphs[0], "new weight values must not cost a capture"
            assert graphs[2] is not graphs[1], "a new label_smoothing must not replay the old capture"
            # the new label_smoothing is in effect: the plan's loss job on the plan's logits
            pl, eng = step.plan, model._get_engine()
            assert pl.loss_opts.label_smoothing == 0.1 and len(eng.plans) == 2
        step.close()
        runs.append(out)
    for k, (a, b) in enumerate(zip(*runs)):
        assert bool(torch.isfinite(a[0]).all())
        for what, x, y in zip(("loss", "n_correct", "dlogits", "grads", "params"), a, b):
            assert torch.equal(x, y) and (x.dtype != F32 or _same_bits(x, y)), (k, what)
    assert not torch.equal(runs[0][0][4], runs[0][1][4]), "the optimizer did not move the parameters"
    # steps 1 and 2 differ in label_smoothing alone -- had the step replayed the stale capture, the eager run would disagree above;
    # and the eager run itself follows the option: its dlogits under 0.3 are the stand-alone kernel's on a fresh model's first step
    model = _model(pkg)
    model.set_loss_options(weight=W_B, ignore_index=-100, label_smoothing=0.3)
    step = pkg.GraphedStep(model, pkg.Adam(model.parameters(), lr=LR), B, S, use_graph=True)
    ids, image, mask, labels = _batch(model.config, B, S, 62, ignore=True)
    step.load_batch(ids, image, mask, labels)
    step.step()
    torch.cuda.synchronize()
    want_loss, want_dl = torch.empty(1, device="cuda"), torch.empty((B, model.config.num_classes), device="cuda")
    pkg.ops.ce_opts_fwd_bwd(step.plan.buf["logits"].clone(), labels, want_loss, want_dl, None, class_weight=torch.tensor(W_B, device="cuda"),
                            ignore_index=-100, label_smoothing=0.3, grad_scale_dev=model._get_engine().loss_scale)
    torch.cuda.synchronize()
    assert _same_bits(step.plan.buf["loss"], want_loss) and _same_bits(step.plan.buf["dlogits"], want_dl)
    step.close()


def test_label_smoothing_changed_after_a_capture_matches_a_fresh_model(pkg):
    """lr = 0 keeps the parameters where they were, so the step after the change can be held against the FIRST step of a fresh model
    built with the new value, bit for bit."""
    B = 5
    batch = _batch(_model(pkg).config, B, S, 70, ignore=True)
    got = {}
    for name in ("changed", "fresh"):
        model = _model(pkg)
        model.set_loss_options(weight=W_A, ignore_index=-100, label_smoothing=0.1 if name == "changed" else 0.3)
        step = pkg.GraphedStep(model, pkg.Adam(model.parameters(), lr=0.0), B, S)
        step.load_batch(*batch)
        step.step()
        if name == "changed":
            torch.cuda.synchronize()
            before = model.flat_grads.clone()
            model.set_loss_options(weight=W_A, ignore_index=-100, label_smoothing=0.3)
            step.step()
        torch.cuda.synchronize()
        got[name] = (step.plan.buf["loss"].clone(), step.plan.buf["dlogits"].clone(), model.flat_grads.clone())
        step.close()
    assert not torch.equal(before, got["changed"][2]), "label_smoothing 0.1 -> 0.3 changed nothing"
    for a, b in zip(got["changed"], got["fresh"]):
        assert _same_bits(a, b)


def test_accumulation_window_under_the_weighted_loss(pkg):
    """Two micro-batches of 3 and 5 rows, class-weighted criterion on the autograd route: .grad is the f32 sum of the two
    single-backward gradients, bit for bit; each micro-batch is normalised by its own weight sum, as torch does."""
    model = _model(pkg)
    crit = pkg.CrossEntropyLoss(weight=W_A, ignore_index=-100, label_smoothing=0.1).cuda()
    mbs = [_batch(model.config, 3, 12, 80, ignore=True), _batch(model.config, 5, 8, 81, ignore=True)]
    alone = []
    for ids, image, mask, labels in mbs:
        model.flat_grads.zero_()
        (crit(model(ids, image, mask), labels) * 0.5).backward()
        torch.cuda.synchronize()
        alone.append(model.flat_grads.clone())
    assert all(bool(torch.isfinite(a).all()) and float(a.abs().sum()) > 0 for a in alone)
    want = alone[0] + alone[1]
    model.set_grad_accumulation(True)
    opt = pkg.Adam(model.parameters(), lr=LR)
    opt.zero_grad()
    for ids, image, mask, labels in mbs:
        (crit(model(ids, image, mask), labels) * 0.5).backward()
    torch.cuda.synchronize()
    assert _same_bits(model.flat_grads, want)
    # the loss of a micro-batch is torch's weighted mean over ITS kept rows
    ids, image, mask, labels = mbs[1]
    with torch.no_grad():
        logits = model(ids, image, mask)
        got = crit(logits, labels)
    loss_r, lbar, _, _, nc_r = _ce_opts_ref(logits.cpu().to(F64), labels.cpu(), torch.tensor(W_A, dtype=F32).to(F64), -100,
                                            float(np.float32(0.1)), "mean", 1.0)
    _check("micro-batch loss", got.reshape(1), loss_r.reshape(1), lbar)
    assert int(crit.last_correct) == nc_r
