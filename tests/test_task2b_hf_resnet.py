"""The organizers' Subtask-2B model (ResNet_example_task2B.py:146-167: a ``transformers.ResNetConfig``-built, two-stage grayscale ResNet) on
the HIP tower -- the CPU half: parameter count, transformers' state_dict key for key, the refusals, the float64 restatement the GPU tests
(tests/test_task2b_hf_resnet_gpu.py) measure against pinned to the library's own module, the input-gradient routes of the narrow layers,
Pillow's L formula on every colour, and the torchvision-keyed towers left as they were."""
import hashlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64

# the three configurations of the model tests (ResNetConfig keywords)
CONFIGS = {
    "example": dict(num_channels=1, layer_type="basic", depths=[2, 2], hidden_sizes=[32, 64], embedding_size=64, num_labels=2),
    "bottleneck": dict(num_channels=3, layer_type="bottleneck", depths=[1, 1], hidden_sizes=[64, 128], embedding_size=32, num_labels=2),
    "default": dict(),
}
SHAPES = {"64x64": (64, 64), "60x52": (60, 52)}


@pytest.fixture(scope="module")
def pkg():
    import multimodal_propaganda_meme_classification_amd as m
    return m


def _hf(name):
    from transformers import ResNetConfig, ResNetForImageClassification
    cfg = ResNetConfig(**CONFIGS[name])
    return cfg, ResNetForImageClassification(cfg)


# ---------------------------------------------------------------------------------------------------------------------
# the float64 restatement (shared with the GPU tests)
# ---------------------------------------------------------------------------------------------------------------------

class RoundSTE(torch.autograd.Function):
    """x -> x rounded to the 16-bit storage type, straight-through (tests/test_basic_resnet_gpu.py Part B's, restated).  `gscale` > 0: an
    ACTIVATION, whose gradient the tower stores in 16 bits too (its gradient stream, scaled by `gscale`): the incoming gradient is rounded
    the same way.  0: a weight -- its gradient is produced in f32."""

    @staticmethod
    def forward(ctx, x, dtype, gscale):
        ctx.dtype, ctx.gscale = dtype, gscale
        return x.to(dtype).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        if ctx.gscale:
            g = (g * ctx.gscale).to(ctx.dtype).to(g.dtype) / ctx.gscale
        return g, None, None


def ref_logits(p, st, image, cfg, training, storage=None):
    """transformers' ResNetForImageClassification over its own state_dict keys, as a composition of F.conv2d / F.batch_norm / max pool / mean /
    linear in the arithmetic of its operands (float64: the reference).  `cfg`: dict(layer_type, depths, downsample_in_first_stage).
    `storage`: the tower's 16-bit storage points, straight-through -- forward: weights, convolution inputs and outputs, BatchNorm (+ residual)
    (+ ReLU) outputs; backward: the gradients of those activations (x 8192 in fp16).  `st`: running statistics, updated in place when training."""
    gs = 8192.0 if storage == F16 else 1.0
    q = (lambda t: RoundSTE.apply(t, storage, gs)) if storage is not None else (lambda t: t)
    qw = (lambda t: RoundSTE.apply(t, storage, 0.0)) if storage is not None else (lambda t: t)

    def conv(x, pfx, **kw):
        return q(F.conv2d(q(x), qw(p[pfx + ".convolution.weight"]), **kw))

    def bn(x, pfx):
        n = pfx + ".normalization."
        return F.batch_norm(x, st[n + "running_mean"], st[n + "running_var"], p[n + "weight"], p[n + "bias"], training, 0.1, 1e-5)

    E = "resnet.embedder.embedder"
    x = q(F.relu(bn(conv(image, E, stride=2, padding=3), E)))
    x = F.max_pool2d(x, 3, 2, 1)
    for si, depth in enumerate(cfg["depths"]):
        for li in range(depth):
            L = f"resnet.encoder.stages.{si}.layers.{li}"
            s = (2 if (si > 0 or cfg.get("downsample_in_first_stage", False)) else 1) if li == 0 else 1
            if cfg["layer_type"] == "bottleneck":
                o = q(F.relu(bn(conv(x, L + ".layer.0"), L + ".layer.0")))
                o = q(F.relu(bn(conv(o, L + ".layer.1", stride=s, padding=1), L + ".layer.1")))
                o = bn(conv(o, L + ".layer.2"), L + ".layer.2")
            else:
                o = q(F.relu(bn(conv(x, L + ".layer.0", stride=s, padding=1), L + ".layer.0")))
                o = bn(conv(o, L + ".layer.1", padding=1), L + ".layer.1")
            idn = x
            if (L + ".shortcut.convolution.weight") in p:
                idn = q(bn(conv(x, L + ".shortcut", stride=s), L + ".shortcut"))
            x = q(F.relu(o + idn))
    return F.linear(x.mean(dim=(2, 3)), p["classifier.1.weight"], p["classifier.1.bias"])


def split_state(sd, dtype=F64):
    p = {k: v.detach().cpu().to(dtype) for k, v in sd.items() if "running_" not in k and "num_batches" not in k}
    st = {k: v.detach().cpu().to(dtype).clone() for k, v in sd.items() if "running_" in k}
    return p, st


def ref_step(sd, image, labels, cfg, training=True, storage=None, arith=F64):
    """(logits, loss, {name: gradient}, running statistics after the pass) of one forward + cross entropy + backward of the restatement"""
    p, st = split_state(sd, arith)
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    logits = ref_logits(leaves, st, image.to(arith), cfg, training, storage)
    loss = F.cross_entropy(logits, labels)
    loss.backward()
    return logits.detach(), loss.detach(), {k: v.grad for k, v in leaves.items()}, st


def randomize_affine(module, g):
    """BatchNorm affine parameters and running statistics off their 1 / 0 defaults"""
    for n, prm in module.named_parameters():
        if prm.dim() == 1 and "normalization" in n:
            prm.data = (torch.rand(prm.shape, generator=g) + 0.5) if n.endswith("weight") else torch.randn(prm.shape, generator=g) * 0.2
    for n, buf in module.named_buffers():
        if n.endswith("running_mean"):
            buf.copy_(torch.randn(buf.shape, generator=g) * 0.1)
        elif n.endswith("running_var"):
            buf.copy_(torch.rand(buf.shape, generator=g) + 0.5)


# ---------------------------------------------------------------------------------------------------------------------
# construction
# ---------------------------------------------------------------------------------------------------------------------

def test_the_examples_model_has_183554_parameters(pkg):
    model = pkg.HFResNetForImageClassification(**CONFIGS["example"])
    assert sum(p.numel() for p in model.parameters()) == 183554          # SURVEY section 4's known answer
    cfg, hf = _hf("example")
    assert sum(p.numel() for p in pkg.HFResNetForImageClassification(cfg).parameters()) == sum(p.numel() for p in hf.parameters()) == 183554
    assert "resnet.encoder.stages.0.layers.0.shortcut.convolution.weight" in model.state_dict()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_state_dict_is_transformers_own(pkg, name):
    cfg, hf = _hf(name)
    for model in (pkg.HFResNetForImageClassification(cfg), pkg.HFResNetForImageClassification(**CONFIGS[name]),
                  pkg.HFResNetForImageClassification(cfg.to_dict() | {"unrelated": 1})):
        want, got = hf.state_dict(), model.state_dict()
        assert list(got) == list(want)
        for k in want:
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
    assert [n for n, _ in model.named_parameters()] == [n for n, _ in hf.named_parameters()]
    assert [n for n, _ in model.named_buffers()] == [n for n, _ in hf.named_buffers()]
    assert any(k.endswith("num_batches_tracked") for k in got) and "classifier.1.weight" in got and "classifier.1.bias" in got
    # both strict loads
    randomize_affine(hf, torch.Generator().manual_seed(1))
    r = model.load_state_dict(hf.state_dict(), strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    assert all(torch.equal(v, hf.state_dict()[k]) for k, v in model.state_dict().items())
    with torch.no_grad():
        for prm in model.parameters():
            prm.add_(1.0)
    r = hf.load_state_dict(model.state_dict(), strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in hf.state_dict().items())
    # the tower walks every convolution once, and its parameters are the model's but the classifier's
    assert len(model.resnet._units) == sum(1 for m in hf.modules() if isinstance(m, torch.nn.Conv2d))
    assert {id(p) for p in model.resnet._tower_params} == {id(p) for n, p in model.named_parameters() if not n.startswith("classifier.")}


@pytest.mark.parametrize("kw, named", [
    (dict(hidden_act="gelu"), "hidden_act"),
    (dict(layer_type="bottleneck", downsample_in_bottleneck=True), "downsample_in_bottleneck"),
    (dict(num_channels=2), "num_channels"),
    (dict(num_channels=4), "num_channels"),
    (dict(embedding_size=60), "embedding_size"),
    (dict(layer_type="basic", hidden_sizes=[32, 68], depths=[1, 1]), "hidden_sizes"),
    (dict(layer_type="bottleneck", hidden_sizes=[64, 48], depths=[1, 1]), "hidden_sizes"),          # 48 // 4 = 12: no multiple of 8
    (dict(layer_type="bottleneck", hidden_sizes=[16], depths=[1]), "hidden_sizes"),                 # 16 // 4 = 4
    (dict(hidden_sizes=[64] * 5, depths=[1] * 5, layer_type="basic"), "hidden_sizes"),              # five stages
    (dict(hidden_sizes=[], depths=[]), "hidden_sizes"),
    (dict(hidden_sizes=[64, 128], depths=[1], layer_type="basic"), "depths"),
    (dict(layer_type="wide"), "layer_type"),
    (dict(compute_dtype="fp32"), "compute_dtype"),
])
def test_refusals_name_the_field(pkg, kw, named):
    with pytest.raises(ValueError, match=named):
        pkg.HFResNetForImageClassification(**kw)
    from transformers import ResNetConfig
    cfg_kw = {k: v for k, v in kw.items() if k != "compute_dtype"}
    if "layer_type" not in kw or kw["layer_type"] in ("basic", "bottleneck"):
        with pytest.raises(ValueError, match=named):
            pkg.HFResNetForImageClassification(ResNetConfig(**cfg_kw), **{k: v for k, v in kw.items() if k == "compute_dtype"})


def test_supported_fields_build(pkg):
    m = pkg.HFResNetForImageClassification(num_channels=3, embedding_size=16, hidden_sizes=[8, 16, 24, 40], depths=[1, 2, 1, 1], layer_type="basic",
                                           downsample_in_first_stage=True, num_labels=5, compute_dtype="bf16", grad_stream_scale=4.0,
                                           options=pkg.TowerOptions(pair_dgrad=False), seed=3)
    assert m.resnet.gscale == 4.0 and m.resnet.options.pair_dgrad is False and m.classifier[1].out_features == 5 and m.resnet.in_channels == 3
    assert m.resnet._block_units[0].conv1.conv.stride == 2 and m.resnet._block_units[0].downsample is not None
    a = pkg.HFResNetForImageClassification(**CONFIGS["example"], seed=3).state_dict()
    b = pkg.HFResNetForImageClassification(**CONFIGS["example"], seed=3).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    with pytest.raises(TypeError, match="nonsense"):
        pkg.HFResNetForImageClassification(nonsense=1)
    with pytest.raises(ValueError, match="pixel_values"):
        m(labels=torch.zeros(1, dtype=torch.long))
    with pytest.raises(pkg._lib.MemehipError):          # no CPU fallback
        m(pixel_values=torch.zeros(1, 3, 32, 32))


# ---------------------------------------------------------------------------------------------------------------------
# the restatement is the library's module
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", ["example", "bottleneck"])
def test_float64_restatement_equals_transformers(name, shape, training):
    """storage off: logits, loss, every parameter gradient and the running statistics equal transformers' module in .double(), to 1e-10
    relative (per tensor, in the maximum norm)"""
    cfg, hf = _hf(name)
    g = torch.Generator().manual_seed(5)
    randomize_affine(hf, g)
    hf = hf.double().train(training)
    H, W = SHAPES[shape]
    image = torch.randn((3, cfg.num_channels, H, W), generator=g, dtype=F64)
    labels = torch.tensor([0, 1, 1])
    sd = {k: v.clone() for k, v in hf.state_dict().items()}
    logits, loss, grads, st = ref_step(sd, image, labels, CONFIGS[name], training=training)
    out = hf(pixel_values=image, labels=labels)
    out.loss.backward()

    def close(a, b, what):
        assert a.shape == b.shape, what
        assert float((a - b).abs().max()) <= 1e-10 * max(float(b.abs().max()), 1e-300), what
    close(logits, out.logits.detach(), "logits")
    close(loss, out.loss.detach(), "loss")
    named = dict(hf.named_parameters())
    assert set(grads) == set(named)
    for k, prm in named.items():
        close(grads[k], prm.grad, k)
    after = hf.state_dict()
    for k, v in st.items():
        close(v, after[k], k)
        assert torch.equal(v, sd[k]) != training, k          # train mode moved them, eval mode did not


# ---------------------------------------------------------------------------------------------------------------------
# routes
# ---------------------------------------------------------------------------------------------------------------------

def _walk(tower, H, W):
    """[(block index, role, _Conv, input h, w)] of every convolution behind the stem"""
    h, w = tower._stem_unit.conv.out_hw(H, W)
    h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    out = []
    for bi, b in enumerate(tower._block_units):
        hh, ww = h, w
        for j, u in enumerate(b.chain):
            out.append((bi, f"layer.{j}", u.conv, hh, ww))
            hh, ww = u.conv.out_hw(hh, ww)
        if b.downsample is not None:
            out.append((bi, "shortcut", b.downsample.conv, h, w))
        h, w = hh, ww
    return out


def test_every_convolution_of_the_example_has_a_route(pkg):
    R = pkg.resnet
    tower = pkg.HFResNetForImageClassification(**CONFIGS["example"]).resnet
    opts = tower.options
    want = {
        (224, 224): {(0, "layer.0"): R.COL2IM, (0, "layer.1"): R.COL2IM, (0, "shortcut"): R.GEMM, (1, "layer.0"): R.COL2IM, (1, "layer.1"): R.COL2IM,
                     (2, "layer.0"): R.IMPLICIT, (2, "layer.1"): R.IMPLICIT, (2, "shortcut"): R.COL2IM, (3, "layer.0"): R.IMPLICIT,
                     (3, "layer.1"): R.IMPLICIT},
        (60, 52): {(0, "layer.0"): R.COL2IM, (0, "layer.1"): R.COL2IM, (0, "shortcut"): R.GEMM, (1, "layer.0"): R.COL2IM, (1, "layer.1"): R.COL2IM,
                   (2, "layer.0"): R.COL2IM, (2, "layer.1"): R.IMPLICIT, (2, "shortcut"): R.COL2IM, (3, "layer.0"): R.IMPLICIT,
                   (3, "layer.1"): R.IMPLICIT},
    }
    maps = {(224, 224): (56, 56), (60, 52): (15, 13)}
    for (H, W), routes in want.items():
        walk = _walk(tower, H, W)
        assert len(walk) == 10 and len(tower._units) == 11
        got = {(bi, role): R.dgrad_route(cv, h, w, opts) for bi, role, cv, h, w in walk}
        assert all(r in (R.GEMM, R.IMPLICIT, R.COL2IM) for r in got.values()) and got == routes, (H, W, got)
        by = {(bi, role): (cv, h, w) for bi, role, cv, h, w in walk}
        c1, h, w = by[(2, "layer.0")]
        ds = by[(2, "shortcut")][0]
        assert (h, w) == maps[(H, W)] and (c1.cin, c1.cout, c1.kh, c1.stride) == (32, 64, 3, 2) and (ds.cin, ds.cout, ds.kh, ds.stride) == (32, 64, 1, 2)
        assert R.pairs_with(c1, ds, h, w, opts) == (H == 224)          # stage 1's strided conv1 + shortcut: on the even map only
        assert not R.pairs_with(c1, ds, h, w, R.TowerOptions(pair_dgrad=False))
        c0, h0, w0 = by[(0, "layer.0")]
        assert not R.pairs_with(c0, by[(0, "shortcut")][0], h0, w0, opts)          # stage 0's shortcut has stride 1
    stem = tower._stem_unit.conv
    assert (stem.cin, stem.cp, stem.ldk, stem.cout) == (1, 8, 7 * 7 * 8 // 64 * 64 + 64, 64)


# ---------------------------------------------------------------------------------------------------------------------
# Pillow's L
# ---------------------------------------------------------------------------------------------------------------------

def test_luma_formula_is_pillows_on_every_colour(pkg):
    from PIL import Image
    v = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([(v >> 16) & 0xFF, (v >> 8) & 0xFF, v & 0xFF], -1).astype(np.uint8).reshape(4096, 4096, 3)
    want = np.asarray(Image.fromarray(rgb, "RGB").convert("L"))
    got = pkg.data.luma_u8_reference(rgb)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)


def test_pipeline_arguments(pkg):
    D = pkg.data
    with pytest.raises(ValueError, match="augment"):
        D.DeviceImagePipeline(grayscale=True, augment=True, mean=(0.45,), std=(0.22,), device="cpu")
    with pytest.raises(ValueError, match="mean"):
        D.DeviceImagePipeline(grayscale=True, device="cpu")          # the ImageNet triples do not fit one band
    with pytest.raises(ValueError, match="mean"):
        D.DeviceImagePipeline(mean=(0.45,), std=(0.22,), device="cpu")
    p = D.DeviceImagePipeline(device="cpu")
    assert p.mean == D.IMAGENET_MEAN and p.std == D.IMAGENET_STD and p.grayscale is False
    p = D.DeviceImagePipeline(grayscale=True, mean=(0.45,), std=(0.22,), device="cpu")
    assert p.mean == (0.45,) and p.std == (0.22,)
    with pytest.raises(pkg._lib.MemehipError):
        p([np.zeros((4, 4, 3), np.uint8)])


# ---------------------------------------------------------------------------------------------------------------------
# the torchvision-keyed towers are what they were
# ---------------------------------------------------------------------------------------------------------------------

# the convolutions in launch order (`_units`; every one followed by its BatchNorm: convN -> bnN, downsample.0 -> downsample.1)
UNITS = {
    "ResNet18": """conv1 layer1.0.conv1 layer1.0.conv2 layer1.1.conv1 layer1.1.conv2 layer2.0.conv1 layer2.0.conv2 layer2.0.downsample.0
        layer2.1.conv1 layer2.1.conv2 layer3.0.conv1 layer3.0.conv2 layer3.0.downsample.0 layer3.1.conv1 layer3.1.conv2 layer4.0.conv1
        layer4.0.conv2 layer4.0.downsample.0 layer4.1.conv1 layer4.1.conv2""",
    "ResNet34": """conv1 layer1.0.conv1 layer1.0.conv2 layer1.1.conv1 layer1.1.conv2 layer1.2.conv1 layer1.2.conv2 layer2.0.conv1 layer2.0.conv2
        layer2.0.downsample.0 layer2.1.conv1 layer2.1.conv2 layer2.2.conv1 layer2.2.conv2 layer2.3.conv1 layer2.3.conv2 layer3.0.conv1
        layer3.0.conv2 layer3.0.downsample.0 layer3.1.conv1 layer3.1.conv2 layer3.2.conv1 layer3.2.conv2 layer3.3.conv1 layer3.3.conv2
        layer3.4.conv1 layer3.4.conv2 layer3.5.conv1 layer3.5.conv2 layer4.0.conv1 layer4.0.conv2 layer4.0.downsample.0 layer4.1.conv1
        layer4.1.conv2 layer4.2.conv1 layer4.2.conv2""",
    "ResNet50": """conv1 layer1.0.conv1 layer1.0.conv2 layer1.0.conv3 layer1.0.downsample.0 layer1.1.conv1 layer1.1.conv2 layer1.1.conv3
        layer1.2.conv1 layer1.2.conv2 layer1.2.conv3 layer2.0.conv1 layer2.0.conv2 layer2.0.conv3 layer2.0.downsample.0 layer2.1.conv1
        layer2.1.conv2 layer2.1.conv3 layer2.2.conv1 layer2.2.conv2 layer2.2.conv3 layer2.3.conv1 layer2.3.conv2 layer2.3.conv3 layer3.0.conv1
        layer3.0.conv2 layer3.0.conv3 layer3.0.downsample.0 layer3.1.conv1 layer3.1.conv2 layer3.1.conv3 layer3.2.conv1 layer3.2.conv2
        layer3.2.conv3 layer3.3.conv1 layer3.3.conv2 layer3.3.conv3 layer3.4.conv1 layer3.4.conv2 layer3.4.conv3 layer3.5.conv1 layer3.5.conv2
        layer3.5.conv3 layer4.0.conv1 layer4.0.conv2 layer4.0.conv3 layer4.0.downsample.0 layer4.1.conv1 layer4.1.conv2 layer4.1.conv3
        layer4.2.conv1 layer4.2.conv2 layer4.2.conv3""",
}
# the input-gradient routes at 224 x 224 of the convolutions behind the stem, in that order: I implicit, G GEMM, C GEMM + col2im, P the
# col2im route replaced by the pair launch (pairs_with)
ROUTES = {
    "ResNet18": "IIII IIP II IIP II IIP II",
    "ResNet34": "IIIIII IIP IIIIII IIP IIIIIIIIII IIP IIII",
    "ResNet50": "IIII IIIIII IIIC IIIIIIIII IIIC IIIIIIIIIIIIIII IIIC IIIIII",
}
# sha256 of the state_dict keys joined by newlines, as the commit before this test gave them
KEYS_SHA = {"ResNet18": (122, "779447cf0a59dec8"), "ResNet34": (218, "5aa6d4978ba3a10a"), "ResNet50": (320, "8f960d1d00758a98")}


def _bn_of(conv_name):
    if conv_name.endswith("downsample.0"):
        return conv_name[:-1] + "1"
    head, _, last = conv_name.rpartition("conv")
    return f"{head}bn{last}"


@pytest.mark.parametrize("arch", list(UNITS))
def test_torchvision_keyed_towers_are_unchanged(pkg, arch):
    R = pkg.resnet
    net = getattr(pkg, arch)(num_classes=10)
    names = {id(m): n for n, m in net.named_modules()}
    convs = UNITS[arch].split()
    assert [names[id(u.conv.mod)] for u in net._units] == convs
    assert [names[id(u.bn.mod)] for u in net._units] == [_bn_of(c) for c in convs]
    # the state_dict: every unit's convolution weight and its BatchNorm's five entries, module by module, then the classifier
    keys = list(net.state_dict())
    expect = set()
    for c in convs:
        expect |= {c + ".weight"} | {f"{_bn_of(c)}.{f}" for f in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")}
    assert set(keys) == expect | {"fc.weight", "fc.bias"} and keys[:2] == ["conv1.weight", "bn1.weight"] and keys[-2:] == ["fc.weight", "fc.bias"]
    assert (len(keys), hashlib.sha256("\n".join(keys).encode()).hexdigest()[:16]) == KEYS_SHA[arch]
    assert [id(p) for p in net._tower_params] == [id(p) for n, p in net.named_parameters() if not n.startswith("fc.")]
    # routes
    letter = {R.IMPLICIT: "I", R.GEMM: "G", R.COL2IM: "C"}
    got = []
    for bi, role, cv, h, w in _walk(net, 224, 224):
        r = letter[R.dgrad_route(cv, h, w, net.options)]
        if role == "shortcut" and R.pairs_with(net._block_units[bi].conv1.conv, cv, h, w, net.options):
            assert r == "C"
            r = "P"
        got.append(r)
    assert "".join(got) == ROUTES[arch].replace(" ", "")
    stem = net._stem_unit.conv
    assert (stem.cin, stem.cp, stem.cout, net.in_channels, net.feature_dim) == (3, 8, 64, 3, 2048 if arch == "ResNet50" else 512)
