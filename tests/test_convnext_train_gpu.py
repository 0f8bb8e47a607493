"""ConvNeXt-tiny as a TRAINABLE image tower (convnext.ConvNeXtTiny.tower, KevinMultimodalClassifier(image="convnext_tiny")).

Kernels, by name: mh_dwconv_nhwc_dgrad and mh_dwconv_nhwc_wgrad (+ the host-only size query mh_dwconv_wgrad_workspace_elems) exact on
small integers against torch.nn.grad on the CPU; mh_layer_scale_bwd against float64 inside a derived bound.  Tower: every parameter's
gradient against the float64 oracle (oracle/convnext_oracle.py under torch.autograd), held to 4x the error of a float32 CPU emulation
that rounds to the 16-bit type where the tower stores (the oracle's ``storage=`` hook; its casts round the gradient stream at the same
points on the way back).  Model: one focal-loss + fused-Adam step of the Kevin classifier over the tower.

Measured on an MI355X, per-parameter  ||g - g64||_F / ||g64||_F  (tests/conftest.parity_log lines ``[convnext tower <dtype>]``): HIP
2.0e-4 ... 1.2e-3 (fp16) and 1.6e-3 ... 1.1e-2 (bf16), the largest HIP / emulation ratio 1.13 / 1.16 against the bound of 4."""
import functools

import pytest
import torch

from conftest import parity_log
from oracle import convnext_oracle as co

pytestmark = pytest.mark.gpu

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
SHAPES = [(2, 96, 56, 56), (3, 192, 28, 28), (2, 384, 14, 14), (2, 768, 7, 7), (1, 16, 9, 13), (2, 200, 5, 8)]
# + a batch whose 245 units exceed every slab count tried below one unit per workgroup, and one where a workgroup DOES walk two units
# (384 channels = 4 chunks -> 128 slabs for 147 units)
WGRAD_SHAPES = SHAPES + [(5, 96, 56, 56), (3, 384, 56, 56)]


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import multimodal_propaganda_meme_classification_amd as m
    return m


def _kind(T16):
    return "fp16" if T16 == F16 else "bf16"


def _nhwc(t, T16):
    return t.permute(0, 2, 3, 1).contiguous().to(T16).cuda()


@functools.lru_cache(maxsize=None)
def _int_case(shape):
    """integer operands and the CPU references of one shape (shared by the dtypes; never modified)"""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(B * 1000 + C + H)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).to(F32)
    w = ri(-1, 1, C, 1, 7, 7)
    dy2, add = ri(-2, 2, B, C, H, W), ri(-3, 3, B, C, H, W)
    dx = torch.nn.grad.conv2d_input((B, C, H, W), w, dy2, padding=3, groups=C)
    x, dy1 = ri(-2, 2, B, C, H, W), ri(-1, 1, B, C, H, W)
    dw = torch.nn.grad.conv2d_weight(x, (C, 1, 7, 7), dy1, padding=3, groups=C)
    return dict(w=w, dy2=dy2, add=add, dx=dx, x=x, dy1=dy1, dw=dw, db=dy1.sum(dim=(0, 2, 3)))


@pytest.mark.parametrize("T16", [F16, BF16])
@pytest.mark.parametrize("shape", SHAPES)
def test_dgrad_is_exact_on_integers(pkg, T16, shape):
    """mh_dwconv_nhwc_dgrad: |dx| <= 49 * 2 + 3 = 101 is exact in f32 and in both 16-bit types; with and without the addend"""
    ops, lib = pkg.ops, pkg._lib.load(_kind(T16))
    B, C, H, W = shape
    c = _int_case(shape)
    wt = torch.empty((49, C), dtype=F32, device="cuda")
    wsrc = c["w"].cuda()
    assert lib.mh_dwconv_weight_pack(wsrc.data_ptr(), wt.data_ptr(), C, 7, torch.cuda.current_stream().cuda_stream) == 0
    dy, add = _nhwc(c["dy2"], T16), _nhwc(c["add"], T16)
    for addend, want in ((None, c["dx"]), (add, c["dx"] + c["add"])):
        dx = torch.full((B * H * W, C), float("nan"), dtype=T16, device="cuda")
        ops.dwconv_dgrad(dy.view(B * H * W, C), wt, B, H, W, addend=None if addend is None else addend.view(B * H * W, C), dx=dx)
        got = dx.view(B, H, W, C).permute(0, 3, 1, 2).float().cpu()
        assert torch.equal(got, want), (shape, addend is not None, float((got - want).abs().max()))


def test_dgrad_and_wgrad_refuse_other_filters_and_channel_counts(pkg):
    lib, st = pkg._lib.load("bf16"), torch.cuda.current_stream().cuda_stream
    a = torch.zeros(2 * 8 * 8 * 16, dtype=BF16, device="cuda")
    wt, dw = torch.zeros(49 * 16, dtype=F32, device="cuda"), torch.zeros(16 * 49, dtype=F32, device="cuda")
    for C, K in ((16, 3), (12, 7)):
        assert lib.mh_dwconv_nhwc_dgrad(a.data_ptr(), wt.data_ptr(), None, a.data_ptr(), 2, 8, 8, C, K, st) != 0
        assert lib.mh_dwconv_wgrad_workspace_elems(2, 8, 8, C, K) == 0
        assert lib.mh_dwconv_nhwc_wgrad(a.data_ptr(), a.data_ptr(), dw.data_ptr(), None, wt.data_ptr(), 2, 8, 8, C, K, 1.0, 0, st) != 0
    assert lib.mh_dwconv_wgrad_workspace_elems(2, 8, 8, 16, 7) > 0


@pytest.mark.parametrize("T16", [F16, BF16])
@pytest.mark.parametrize("shape", WGRAD_SHAPES)
def test_wgrad_and_dbias_are_exact_on_integers(pkg, T16, shape):
    """mh_dwconv_nhwc_wgrad: dy in [-1, 1], x in [-2, 2] -- the largest sum is 2 B H W <= 31 360 < 2^24, every partial exact in f32 whatever
    the slab order; scale 0.5, accumulation into a pre-filled buffer, two runs bit for bit, the workspace check of the wrapper"""
    ops = pkg.ops
    B, C, H, W = shape
    c = _int_case(shape)
    x, dy = _nhwc(c["x"], T16).view(B * H * W, C), _nhwc(c["dy1"], T16).view(B * H * W, C)
    need = ops.dwconv_wgrad_workspace_elems(B, H, W, C)
    assert need >= 50 * C and need % (50 * C) == 0
    nan = lambda *s: torch.full(s, float("nan"), dtype=F32, device="cuda")
    dw, db = nan(C, 1, 7, 7), nan(C)
    ops.dwconv_wgrad(x, dy, dw, db, B, H, W, workspace=nan(need))
    assert torch.equal(dw.cpu(), c["dw"]) and torch.equal(db.cpu(), c["db"]), (float((dw.cpu() - c["dw"]).abs().max()), float((db.cpu() - c["db"]).abs().max()))
    dw2, db2 = nan(C, 1, 7, 7), nan(C)
    ops.dwconv_wgrad(x, dy, dw2, db2, B, H, W)
    assert torch.equal(dw2, dw) and torch.equal(db2, db)                                   # run to run
    ops.dwconv_wgrad(x, dy, dw2, db2, B, H, W, scale=0.5)
    assert torch.equal(dw2.cpu(), c["dw"] * 0.5) and torch.equal(db2.cpu(), c["db"] * 0.5)
    pre_w = torch.arange(C * 49, dtype=F32).view(C, 1, 7, 7) % 17 - 8
    pre_b = torch.arange(C, dtype=F32) % 5
    dw3, db3 = pre_w.cuda(), pre_b.cuda()
    ops.dwconv_wgrad(x, dy, dw3, db3, B, H, W, accum=True)
    assert torch.equal(dw3.cpu(), pre_w + c["dw"]) and torch.equal(db3.cpu(), pre_b + c["db"])
    ops.dwconv_wgrad(x, dy, dw3, None, B, H, W)                                             # no bias gradient asked for
    assert torch.equal(dw3, dw)
    with pytest.raises(ValueError, match="workspace"):
        ops.dwconv_wgrad(x, dy, dw3, db3, B, H, W, workspace=torch.empty(need - 1, dtype=F32, device="cuda"))


@pytest.mark.parametrize("C,K", [(96, 384), (768, 3072)])
def test_layer_scale_bwd_matches_float64(pkg, C, K):
    """mh_layer_scale_bwd.  dgamma is a K+1-term f32 sum in some order: |err| <= (K + 1) 2^-24 (sum_k |W dW'| + |b db'|) per row (the
    standard bound of a recursive sum of rounded products).  dW = gamma dW', db = gamma db' in place: ONE f32 rounding, so equal to the
    CPU's f32 product.  Accumulating form: the product may be fused into the add, so one more rounding of the sum is allowed."""
    ops = pkg.ops
    g = torch.Generator().manual_seed(C)
    W, dWp = torch.randn((C, K), generator=g), torch.randn((C, K), generator=g)
    b, dbp, gamma = torch.randn(C, generator=g), torch.randn(C, generator=g), 0.3 * (0.5 + torch.rand(C, generator=g))
    ref = (W.double() * dWp.double()).sum(1) + b.double() * dbp.double()
    bound = (K + 1) * 2.0 ** -24 * ((W.double() * dWp.double()).abs().sum(1) + (b.double() * dbp.double()).abs())
    dW, db, dgam = dWp.clone().cuda(), dbp.clone().cuda(), torch.full((C,), float("nan"), device="cuda")
    ops.layer_scale_bwd(W.cuda(), b.cuda(), gamma.cuda(), dW, db, dgam)
    err = (dgam.cpu().double() - ref).abs()
    parity_log(f"[layer_scale_bwd C={C} K={K}] max |dgamma - f64| / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(dW.cpu(), gamma[:, None] * dWp) and torch.equal(db.cpu(), gamma * dbp)
    # accumulate into buffers of their own
    oW, ob, og = torch.randn((C, K), generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g)
    aW, ab, ag = oW.clone().cuda(), ob.clone().cuda(), og.clone().cuda()
    ops.layer_scale_bwd(W.cuda(), b.cuda(), gamma.cuda(), dWp.cuda(), dbp.cuda(), ag, dW=aW, db=ab, accum=True)
    u = 2.0 ** -23
    wantW = oW.double() + gamma.double()[:, None] * dWp.double()
    assert bool(((aW.cpu().double() - wantW).abs() <= u * (oW.abs() + (gamma[:, None] * dWp).abs()).double()).all())
    assert bool(((ab.cpu().double() - (ob.double() + gamma.double() * dbp.double())).abs() <= u * (ob.abs() + (gamma * dbp).abs()).double()).all())
    assert bool(((ag.cpu().double() - (og.double() + ref)).abs() <= bound + u * (og.abs().double() + ref.abs())).all())
    with pytest.raises(ValueError):
        ops.layer_scale_bwd(W.cuda(), b.cuda(), gamma.cuda(), dW, db, dgam, accum=True)      # in place cannot accumulate


# ---- the whole tower ------------------------------------------------------------------------------------------------------------
DEPTHS, DIMS = (1, 1, 2, 1), co.DIMS


def _oracle_grads(p, x, r, dtype, storage=None):
    q = {k: v.detach().to(dtype).requires_grad_(True) for k, v in p.items() if k.startswith("features.")}
    out = co.convnext_pooled_features(q, x.to(dtype), DEPTHS, DIMS, storage=storage)
    (out * r.to(dtype)).sum().backward()
    return out.detach(), {k: v.grad.double() for k, v in q.items()}


@pytest.fixture(scope="module")
def tower_case():
    g = torch.Generator().manual_seed(11)
    p = co.init_params(seed=5, depths=DEPTHS, dims=DIMS)
    x, r = torch.randn((2, 3, 64, 64), generator=g), torch.randn((2, DIMS[-1]), generator=g)
    out64, g64 = _oracle_grads(p, x, r, F64)
    return dict(p=p, x=x, r=r, out64=out64, g64=g64)


def _rel(g, g64):
    return float((g.double() - g64).norm() / g64.norm())


@pytest.mark.parametrize("T16", [F16, BF16])
def test_tower_gradients_match_float64(pkg, tower_case, T16):
    """Every parameter's gradient of (tower(x) * r).sum() against float64, depths (1, 1, 2, 1) at 2 x 64 x 64 (the 96 -> 128 path, three
    downsampling layers, two blocks in one stage, a chunked and an unchunked weight gradient).  Bound per parameter: 4x the same
    metric of the f32 emulation with 16-bit storage points -- the margin is for another summation order, not for a wrong term.  The
    forward equals pooled_features bit for bit; a second backward doubles every .grad exactly (the accumulate-in-place paths)."""
    from multimodal_propaganda_meme_classification_amd.convnext import ConvNeXtTiny
    c = tower_case
    _, gemu = _oracle_grads(c["p"], c["x"], c["r"], F32, storage=T16)
    net = ConvNeXtTiny(compute_dtype=_kind(T16), depths=DEPTHS, dims=DIMS)
    net.load_state_dict(c["p"], strict=True)
    net = net.cuda()
    x, r = c["x"].cuda(), c["r"].cuda()
    out = net.tower(x)
    assert out.dtype == F32 and tuple(out.shape) == (2, net.feature_dim) and net.feature_dim == DIMS[-1]
    assert torch.equal(out.detach(), net.pooled_features(x))
    with torch.no_grad():
        assert torch.equal(net.tower(x), out.detach())
    (out * r).sum().backward()
    named = dict(net.features.named_parameters())
    assert {"features." + k for k in named} == set(c["g64"])
    worst, bad, first = 0.0, [], {}
    for k, p in named.items():
        k = "features." + k
        assert p.grad is not None and p.grad.dtype == F32 and p.grad.shape == p.shape, k
        e_hip, e_emu = _rel(p.grad.cpu(), c["g64"][k]), _rel(gemu[k], c["g64"][k])
        parity_log(f"[convnext tower {_kind(T16)}] {k}: hip {e_hip:.3e} emulation {e_emu:.3e} ratio {e_hip / e_emu:.2f}")
        worst = max(worst, e_hip / e_emu)
        if not e_hip <= 4.0 * e_emu:
            bad.append((k, e_hip, e_emu))
        first[k] = p.grad.clone()
    parity_log(f"[convnext tower {_kind(T16)}] largest hip / emulation ratio over {len(named)} parameters: {worst:.2f} (bound 4)")
    assert not bad, bad
    (net.tower(x) * r).sum().backward()          # every .grad exists now: the kernels accumulate in place
    for k, p in named.items():
        assert torch.equal(p.grad, 2 * first["features." + k]), k
    assert all(p.grad is None for p in net.classifier.parameters())


# ---- the submitted model over the organizers' backbone ----------------------------------------------------------------------------
def _kevin_step(pkg, lr):
    torch.manual_seed(7)
    torch.cuda.manual_seed(7)
    tc = pkg.TextConfig(vocab_size=600, hidden=128, layers=2, heads=2, intermediate=256, max_position=64)
    cc = pkg.TextConfig(vocab_size=500, hidden=128, layers=2, heads=2, intermediate=256, max_position=64)
    model = pkg.KevinMultimodalClassifier("concatenation", text=tc, image="convnext_tiny", caption=cc, proj=128, compute_dtype="fp16", seed=1,
                                          convnext_depths=(1, 1, 1, 1)).cuda()
    with torch.no_grad():          # (fp16: the from-scratch layer_scale of 1e-6 underflows in the folded weight; checkpoints hold ~0.1 ... 1)
        for k, p in model.named_parameters():
            if k.endswith("layer_scale"):
                p.fill_(0.3)
    n, S = 4, 16
    g = torch.Generator().manual_seed(5)
    text, cap = torch.randint(5, 600, (n, S), generator=g), torch.randint(5, 500, (n, S), generator=g)
    mask = (torch.arange(S)[None] < torch.randint(4, S + 1, (n,), generator=g)[:, None]).long()
    image = torch.randn((n, 3, 64, 64), generator=g)
    labels = torch.tensor([0.0, 1.0, 1.0, 0.0]).cuda()
    batch = [t.cuda() for t in (text * mask, image, mask, cap * mask, mask)]
    model.train()
    opt = pkg.Adam(model.get_params(lr))
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    opt.zero_grad()
    out = model(*batch)
    loss = pkg.SigmoidFocalLoss()(out, labels, alpha=0.25, gamma=2.0, reduction="mean")
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    return model, opt, before, float(loss.detach())


def test_kevin_model_trains_over_convnext_tiny(pkg):
    """KevinMultimodalClassifier(image="convnext_tiny"): one focal-loss + fused-Adam step moves EVERY parameter of the image tower (layer
    scale, depthwise weights and stem by name), the image group runs at 0.8 lr, a second run from the same seed ends in the same bits, and
    a checkpoint under the reference's prefixes (torchvision's convnext_tiny names below image_model.image_model.) round-trips."""
    import math
    from multimodal_propaganda_meme_classification_amd.convnext import ConvNeXtTiny
    lr = 1e-3
    model, opt, before, loss = _kevin_step(pkg, lr)
    assert math.isfinite(loss) and model.towers is None and type(model.image_model) is ConvNeXtTiny
    assert tuple(model.image_fine_tune[0].weight.shape) == (128, 768)
    assert [g["lr"] for g in opt.param_groups] == [lr, lr * 0.8, lr * 0.8]
    image_ids = {id(p) for p in opt.param_groups[2]["params"]}
    after = dict(model.named_parameters())
    tower = [k for k in after if k.startswith("image_model.")]
    assert len(tower) == 4 + 4 * 9 + 3 * 4
    for k in tower + [k for k in after if k.startswith("image_fine_tune.")]:
        assert id(after[k]) in image_ids, k
        assert bool(torch.isfinite(after[k]).all()) and not torch.equal(after[k].detach(), before[k]), k
    for k in ("image_model.features.1.0.layer_scale", "image_model.features.1.0.block.0.weight", "image_model.features.7.0.block.0.weight",
              "image_model.features.0.0.weight", "image_model.features.0.0.bias"):
        assert k in tower and float((after[k].detach() - before[k]).abs().max()) > 0.1 * lr, k
    again, _, _, loss2 = _kevin_step(pkg, lr)
    assert loss2 == loss
    for k, v in again.named_parameters():
        assert torch.equal(v.detach(), after[k].detach()), k
    # checkpoint of the reference module: text_model.model.*, image_model.image_model.<torchvision names>, image_model.fine_tune.*
    pre = (("text_model.", "text_model.model."), ("caption_text_model.", "caption_text_model.model."), ("image_model.", "image_model.image_model."),
           ("image_fine_tune.", "image_model.fine_tune."))
    g = torch.Generator().manual_seed(4)
    want = {k: (torch.randn(v.shape, generator=g) if v.dtype.is_floating_point else v.cpu() + 3) for k, v in model.state_dict().items()}
    ref = {}
    for k, v in want.items():
        for a, b in pre:
            if k.startswith(a):
                k = b + k[len(a):]
                break
        ref[k] = v
    assert "image_model.image_model.features.1.0.layer_scale" in ref and "image_model.image_model.features.2.1.weight" in ref
    ref["image_model.image_model.classifier.2.weight"] = torch.zeros(1000, 768)          # torchvision's head: no counterpart, left out
    res = model.load_reference_state_dict(ref)
    assert not res.missing_keys and not res.unexpected_keys
    got = model.state_dict()
    assert all(torch.equal(got[k].cpu(), want[k]) for k in want)
