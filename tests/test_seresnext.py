"""SE-ResNeXt-50 32x4d: the module tree (timm's ``seresnext50_32x4d``, written out from its published module tree -- timm is not a
dependency), the hidden-width rule, the callers' name lists and the route clause that keeps the block-out epilogue away from a
squeeze-and-excitation block.  CPU only -- nothing here launches a kernel."""
import pytest
import torch

import multimodal_propaganda_meme_classification_amd as pkg
from multimodal_propaganda_meme_classification_amd import resnet as R

SE_KEYS = ("se.fc1.weight", "se.fc1.bias", "se.fc2.weight", "se.fc2.bias")


def _keys(block_counts, with_fc=True, se=False):
    """the state_dict order of a bottleneck ResNet: torchvision's, with timm's four ``se.*`` keys between bn3 and the downsample"""
    def bn(p):
        return [p + s for s in (".weight", ".bias", ".running_mean", ".running_var", ".num_batches_tracked")]
    out = ["conv1.weight"] + bn("bn1")
    for li, n in enumerate(block_counts, 1):
        for bi in range(n):
            L = f"layer{li}.{bi}."
            for k in (1, 2, 3):
                out += [L + f"conv{k}.weight"] + bn(L + f"bn{k}")
            if se:
                out += [L + k for k in SE_KEYS]
            if bi == 0:
                out += [L + "downsample.0.weight"] + bn(L + "downsample.1")
    return out + (["fc.weight", "fc.bias"] if with_fc else [])


def test_seresnext50_has_timms_tree_and_parameter_count():
    with torch.device("meta"):
        net = pkg.SEResNeXt50_32x4d()
    assert sum(p.numel() for p in net.parameters()) == 27_559_896 == 25_028_904 + 2_530_992
    assert list(net.state_dict().keys()) == _keys((3, 4, 6, 3), se=True)
    assert tuple(net.layer1[0].se.fc1.weight.shape) == (16, 256, 1, 1) and tuple(net.layer1[0].se.fc2.weight.shape) == (256, 16, 1, 1)
    assert tuple(net.layer4[2].se.fc1.weight.shape) == (128, 2048, 1, 1) and tuple(net.layer4[2].se.fc2.bias.shape) == (2048,)
    per_block = [sum(p.numel() for p in getattr(net, f"layer{i}")[0].se.parameters()) for i in (1, 2, 3, 4)]
    assert per_block == [8_464, 33_312, 132_160, 526_464]
    assert all(isinstance(b.se, pkg.SEModule) for i in (1, 2, 3, 4) for b in getattr(net, f"layer{i}"))
    assert tuple(net.layer1[0].conv2.weight.shape) == (128, 4, 3, 3) and net.layer3[0].conv2.groups == 32       # still the ResNeXt body
    assert net.feature_dim == 2048 and R.RESNETS["seresnext50_32x4d"] is pkg.SEResNeXt50_32x4d
    tower = {id(p) for p in net._tower_params}
    assert all(id(p) in tower for n, p in net.named_parameters() if ".se." in n) and id(net.fc.weight) not in tower


def test_the_hidden_width_rule_is_timms_make_divisible():
    assert [R.se_reduced_channels(c) for c in (256, 512, 1024, 2048)] == [16, 32, 64, 128]
    assert R.se_reduced_channels(192) == 16 and R.se_reduced_channels(64) == 8
    b = pkg.Bottleneck(64, 48, se=True)          # C = 192
    assert tuple(b.se.fc1.weight.shape) == (16, 192, 1, 1)
    assert [k for k in b.state_dict() if k.startswith("se.")] == list(SE_KEYS)
    assert not hasattr(pkg.Bottleneck(64, 48), "se")


def test_the_existing_towers_are_unchanged():
    with torch.device("meta"):
        x, r = pkg.ResNeXt50_32x4d(), pkg.ResNet50()
    assert sum(p.numel() for p in x.parameters()) == 25_028_904 and list(x.state_dict().keys()) == _keys((3, 4, 6, 3))
    assert sum(p.numel() for p in r.parameters()) == 25_557_032 and list(r.state_dict().keys()) == _keys((3, 4, 6, 3))
    assert all(b.se is None for net in (x, r) for b in net._block_units)


def test_binary_head_model_has_the_references_names():
    m = pkg.SEResNeXt50_32x4d_BH(layers=(1, 1, 1, 1))
    rest = [k for k in m.state_dict() if not k.startswith("net.")]
    assert rest == ["fea_bn.weight", "fea_bn.bias", "fea_bn.running_mean", "fea_bn.running_var", "fea_bn.num_batches_tracked",
                    "binary_head.fc.0.weight", "binary_head.fc.0.bias"]
    assert not hasattr(m, "fc") and isinstance(m.dropout, torch.nn.Dropout) and m.model_arch == "seresnext50_32x4d"
    assert tuple(m.binary_head.fc[0].weight.shape) == (2, 2048) and m.binary_head.s == 1
    assert not m.fea_bn.bias.requires_grad and m.fea_bn.weight.requires_grad
    assert [k[4:] for k in m.state_dict() if k.startswith("net.")] == _keys((1, 1, 1, 1), with_fc=False, se=True)


def test_callers_accept_the_new_name_and_still_name_every_arch():
    for make in (lambda: pkg.KevinMultimodalClassifier(image="nope"), lambda: pkg.ResNetClassifier(arch="nope")):
        with pytest.raises(ValueError) as e:
            make()
        for arch in ("resnet18", "resnet34", "resnext50_32x4d", "seresnext50_32x4d"):
            assert arch in str(e.value), (arch, str(e.value))
    with pytest.raises(ValueError, match="resnet50"):
        pkg.ResNetClassifier(arch="nope")
    with pytest.raises(ValueError, match="convnext_tiny"):
        pkg.KevinMultimodalClassifier(image="nope")
    clf = pkg.ResNetClassifier(arch="seresnext50_32x4d", layers=(1, 1, 1, 1))
    assert type(clf.resnet) is pkg.SEResNeXt50_32x4d and clf.resnet.fc.out_features == 2
    tc = pkg.TextConfig(vocab_size=100, hidden=128, layers=1, heads=2, intermediate=128, max_position=32)
    kev = pkg.KevinMultimodalClassifier("concatenation", text=tc, image="seresnext50_32x4d", caption=tc, proj=128, resnet_layers=(1, 1, 1, 1))
    assert type(kev.image_model) is pkg.SEResNeXt50_32x4d and kev.image_fine_tune[0].in_features == 2048


def _block_out_answers(net, size=64):
    """epilogue_takes_bn(block_out=True) of every conv1 that has a block below it, asked as the backward's block loop asks, on the image sizes
    the forward walk gives (stem / 2, max pool / 2, then each block's stride)"""
    opts = pkg.TowerOptions()
    h, w = net._stem_unit.conv.out_hw(size, size)
    h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    out = []
    for k, blk in enumerate(net._block_units):
        if k:
            below = net._block_units[k - 1]
            out.append((R.epilogue_takes_bn(blk.conv1.conv, h, w, opts, block_out=True, below_se=below.se is not None),
                        R.epilogue_takes_bn(blk.conv1.conv, h, w, opts, block_out=True)))
        for u in blk.chain:
            h, w = u.conv.out_hw(h, w)
    return out


def test_no_conv1_above_an_se_block_takes_the_block_out_epilogue():
    with torch.device("meta"):
        se = pkg.SEResNeXt50_32x4d(layers=(1, 1, 1, 1))
        plain = pkg.ResNeXt50_32x4d(layers=(1, 1, 1, 1))
        full = pkg.ResNeXt50_32x4d()
    got = _block_out_answers(se)
    assert len(got) == 3 and all(b.se is not None for b in se._block_units)
    assert [clause for clause, _ in got] == [False, False, False]
    assert [parent for _, parent in got] == [True, True, True]          # the same conv1 above a plain block would have taken it
    # for the ResNeXt towers the answer with the clause is the answer without it: the parent commit's
    for net in (plain, full):
        answers = _block_out_answers(net, 224)
        assert answers and all(clause == parent for clause, parent in answers) and all(parent for _, parent in answers)
    opts = pkg.TowerOptions()
    c1 = se._block_units[1].conv1.conv
    assert R.epilogue_takes_bn(c1, 16, 16, opts, below_se=True) == R.epilogue_takes_bn(c1, 16, 16, opts)      # (only the block_out form is barred)
